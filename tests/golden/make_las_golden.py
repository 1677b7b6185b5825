"""Writes tests/golden/bunny_8k.las from the laspy-2.5.3-written bunny.las of the
project this package mirrors (its data/bunny.las: LAS 1.2, point format 3,
35,947 records of 34 bytes, scales 1e-4, offsets 0):

    python tests/golden/make_las_golden.py /path/to/data/bunny.las

The fixture is that file's 227-byte header plus its first 8,192 records,
byte for byte, with the legacy point count set to 8192.  The header's min / max
therefore still describe the full file; the tests do not compare them on
reading.  It is the only laspy-written data at hand and pins both directions:
checked here for all 35,947 records, X == np.round(float64(float32 x) / 1e-4)
against tests/golden/bunny.pcd's x / y / z, the other 22 bytes of every record
are zero, nothing trails the point block, and the header's min / max equal
(min or max X) * scale + offset."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
import las_oracle as LO  # noqa: E402

OUT = os.path.join(HERE, "bunny_8k.las")
KEEP = 8192


def main(src: str):
    from open3dpypro.pcd_io import read_pcd_arrays

    with open(src, "rb") as f:
        b = f.read()
    h = LO.read_header(b)
    assert (h["version"], h["format"], h["stride"], h["header_size"], h["data_offset"]) == ((1, 2), 3, 34, 227, 227)
    assert h["count"] == 35947 and len(b) == 227 + h["count"] * 34, "nothing may trail the point block"
    assert np.array_equal(h["scales"], [1e-4] * 3) and np.array_equal(h["offsets"], [0.0] * 3)
    assert h["by_return"] == (0, 0, 0, 0, 0)
    rec = np.frombuffer(b, dtype=LO.record_dtype(3), count=h["count"], offset=227)
    raw = np.frombuffer(b, dtype=np.uint8, offset=227).reshape(h["count"], 34)
    assert not raw[:, 12:].any(), "only X, Y, Z are set"
    fl = read_pcd_arrays(os.path.join(HERE, "bunny.pcd"))
    p = np.stack([fl["x"], fl["y"], fl["z"]], 1).astype(np.float32)
    assert len(p) == h["count"]
    X = np.stack([rec["X"], rec["Y"], rec["Z"]], 1)
    assert np.array_equal(X, LO.quantise(p, h["scales"], h["offsets"]))
    mins, maxs = LO.minmax(X, h["scales"], h["offsets"])  # laspy's header min / max: (min or max X) * scale + offset
    assert np.array_equal(mins, h["mins"]) and np.array_equal(maxs, h["maxs"])
    out = bytearray(b[:227 + KEEP * 34])
    struct.pack_into("<I", out, 107, KEEP)
    with open(OUT, "wb") as f:
        f.write(bytes(out))
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) == 227 + KEEP * 34 < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
