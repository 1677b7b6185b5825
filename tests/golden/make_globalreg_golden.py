"""Writes tests/golden/globalreg_ref.npz: the bunny pair's answers of the numpy
restatement (tests/globalreg_oracle.py) of FPFH, feature matching and RANSAC
on correspondences.

    python tests/golden/make_globalreg_golden.py

Stored: every fourth float32 feature row of both clouds, the mutual
correspondences (int32), the head of the sample list the rule consumed
(ransac_samples(C, 3, 100000, seed), int32), and the rule's outcome on it.

Asserted here — the conditions under which exact or tight comparisons of a
float32 / guard-banded implementation against this float64 restatement stand:
  - no pair feature within 1e-9 bin units of a bin edge;
  - for every pair |a1| and |a2| are bitwise equal or their acos values differ
    by more than 1e-12, and no acos argument exceeds 1;
  - the matcher's relative gap between the best and the runner-up d^2 (float64
    on the float32 features) is exactly 0 or above 1e-5 for every row;
  - for every hypothesis the rule scores, no correspondence within 1e-9 of the
    distance threshold;
  - the rule stops before 100000 iterations within 5 degrees and 0.01 of the
    motion applied, and the CPU oracle's point-to-plane ICP from there ends
    within 0.2 degrees and 5e-4.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
import globalreg_cases as GC  # noqa: E402
import globalreg_oracle as GO  # noqa: E402

OUT = os.path.join(HERE, "globalreg_ref.npz")
ROW_STEP = 4


def bunny_features(pts, normal_param, diag):
    from oracle import oracle as O

    nrm = O.estimate_normals(pts, O.HYBRID, normal_param[1], normal_param[0]).astype(np.float32)
    idx, d2, cnt = O.knn_search(pts, pts, O.HYBRID, GC.BUNNY_FPFH[1], GC.BUNNY_FPFH[0])
    f, _, _ = GO.fpfh(pts, nrm, idx, d2, cnt, diag)
    diag["list_min"], diag["list_max"] = int(cnt.min()), int(cnt.max())
    return nrm, f.astype(np.float32)


def main():
    from open3dpypro.pcd_io import read_pcd_arrays
    from oracle import oracle as O

    fl = read_pcd_arrays(os.path.join(HERE, "bunny.pcd"))
    bunny = np.stack([fl["x"], fl["y"], fl["z"]], 1).astype(np.float32)
    src, tgt, T_true = GC.bunny_pair(bunny)
    print("source", len(src), "target", len(tgt))
    feats = {}
    for name, pts, par in (("src", src, GC.BUNNY_NORMALS_SRC), ("tgt", tgt, GC.BUNNY_NORMALS_TGT)):
        diag = {}
        nrm, f = bunny_features(pts, par, diag)
        print(name, diag)
        assert diag["bin_edge_min"] > 1e-9, diag
        assert diag["acos_gap_min"] > 1e-12, diag
        assert diag["acos_arg_max"] <= 1.0, diag
        feats[name] = (nrm, f)
    fs, ft = feats["src"][1], feats["tgt"][1]
    for a, b, what in ((fs, ft, "forward"), (ft, fs, "backward")):
        _, gap = GO.match(a, b)
        bad = (gap != 0.0) & ~(gap > 1e-5)
        print(what, "smallest non-zero gap", gap[gap > 0].min(), "ties", int((gap == 0).sum()))
        assert not bad.any(), (what, int(bad.sum()))
    corres = GO.correspondences(fs, ft, mutual_filter=True)
    C = len(corres)
    d = GO.transform_dist(T_true, src.astype(np.float64)[corres[:, 0]], tgt.astype(np.float64)[corres[:, 1]])[0]
    print("mutual pairs", C, "within the distance of the truth", int((d < GC.BUNNY_MAX_DIST).sum()))
    assert C < len(src) and C >= 0.1 * len(src)
    samples = O.ransac_samples(C, 3, GC.BUNNY_MAX_ITER, GC.BUNNY_SEED)
    r = GO.ransac(src, tgt, corres, samples, GC.BUNNY_MAX_DIST, 3, GC.BUNNY_EDGE, GC.BUNNY_MAX_DIST, 0.999)
    rot, tr = GC.pose_error(r["T"], T_true)
    print("ransac: processed", r["processed"], "scored", r["scored"], "best", r["best_iteration"], "count", r["count"],
          "pose error", rot, tr, "threshold gap", r["thr_gap_min"])
    assert r["processed"] < GC.BUNNY_MAX_ITER and rot < 5.0 and tr < 0.01
    assert r["thr_gap_min"] > 1e-9
    T, fit, rm, _ = O.registration_icp(src, tgt, feats["tgt"][0], GC.BUNNY_MAX_DIST, init=r["T"])
    rot2, tr2 = GC.pose_error(T, T_true)
    print("icp from there: fitness", fit, "rmse", rm, "pose error", rot2, tr2)
    assert rot2 < 0.2 and tr2 < 5e-4
    keep = min(len(samples), r["processed"] + 8)
    np.savez_compressed(
        OUT, feat_src=fs[::ROW_STEP], feat_tgt=ft[::ROW_STEP], row_step=np.int32(ROW_STEP),
        sizes=np.int32([len(src), len(tgt)]), corres=corres.astype(np.int32), samples=samples[:keep].astype(np.int32),
        seed=np.int64(GC.BUNNY_SEED), T=r["T"], best_iteration=np.int32(r["best_iteration"]),
        processed=np.int32(r["processed"]), scored=np.int32(r["scored"]), count=np.int32(r["count"]),
        err2=np.float64(r["err2"]))
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 400 * 1024


if __name__ == "__main__":
    main()
