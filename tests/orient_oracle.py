"""Numpy restatement of the normal-orientation rule (include/o3dx.h "spanning
trees and consistent normal orientation"; Open3D 0.19
OrientNormalsConsistentTangentPlane(k) with one strict total order on edges).

TEST INFRASTRUCTURE ONLY: dense and quadratic in n, for clouds of a few
thousand points.  Steps, each in the operation order the rule states:
  1. d^2 = ((dx dx) + dy dy) + dz dz in float64 on the float32 coordinates;
  2. kNN lists by sorting (d^2, index), the point itself included;
  3. EMST: Kruskal on the complete graph under (d^2, lo, hi);
  4. Riemannian graph: kNN edges united with the EMST;
  5. Kruskal on it under (1 - |dot|, lo, hi), dot = ((nx nx') + ny ny') + nz nz';
  6. root = lowest index of maximal z, flipped iff nz < 0; along the tree a
     child flips iff dot(parent as oriented, child) < 0.
reverse_ties=True orders equal weights by descending (lo, hi) instead: a
result that does not change under it does not hinge on a tie."""
import numpy as np


def d2_dense(p):
    p = np.asarray(p, np.float32).astype(np.float64)
    dx = p[:, None, 0] - p[None, :, 0]
    r = dx * dx
    dx = p[:, None, 1] - p[None, :, 1]
    r = r + dx * dx
    dx = p[:, None, 2] - p[None, :, 2]
    r = r + dx * dx
    return r


def knn_lists(d2, k):
    """(n, min(k, n)) neighbour indices by (d^2, index); a stable sort of the
    row keeps the lower index first among equal distances."""
    n = len(d2)
    return np.argsort(d2, axis=1, kind="stable")[:, :min(k, n)].astype(np.int32)


def kruskal(n, lo, hi, w, reverse_ties=False):
    """Positions (into lo / hi / w) of the spanning forest's edges under the
    order (w, lo, hi) — (w, -lo, -hi) with reverse_ties — in that order."""
    lo = np.asarray(lo, np.int64)
    hi = np.asarray(hi, np.int64)
    order = np.lexsort((-hi, -lo, w)) if reverse_ties else np.lexsort((hi, lo, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    taken = []
    ll, hh = lo.tolist(), hi.tolist()
    for e in order.tolist():
        a, b = find(ll[e]), find(hh[e])
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(e)
            if len(taken) == n - 1:
                break
    return np.asarray(taken, np.int64)


def sort_edges(e):
    e = np.asarray(e, np.int64).reshape(-1, 2)
    return e[np.lexsort((e[:, 1], e[:, 0]))].astype(np.int32)


def emst(p, d2=None, reverse_ties=False):
    """(n - 1, 2) int32 {lo, hi} rows sorted by (lo, hi).  Kruskal runs on the
    edges up to a weight threshold (every tie at the threshold included) and
    the threshold grows until the tree is complete: the same tree as over all
    edges, since Kruskal only ever looks at a prefix of the sorted list."""
    n = len(p)
    if n < 2:
        return np.zeros((0, 2), np.int32)
    d2 = d2_dense(p) if d2 is None else d2
    lo, hi = np.triu_indices(n, 1)
    w = d2[lo, hi]
    m = min(len(w), 16 * n)
    while True:
        if m >= len(w):
            sel = np.arange(len(w))
        else:
            sel = np.nonzero(w <= np.partition(w, m - 1)[m - 1])[0]
        t = kruskal(n, lo[sel], hi[sel], w[sel], reverse_ties)
        if len(t) == n - 1:
            return sort_edges(np.stack([lo[sel][t], hi[sel][t]], 1))
        assert m < len(w), "the complete graph is connected"
        m = min(len(w), 8 * m)


def knn_edges(knn):
    """Every {i, j != i} of the lists as unique (lo, hi) rows."""
    n, k = knn.shape
    i = np.repeat(np.arange(n), k)
    j = knn.reshape(-1).astype(np.int64)
    keep = (j != i) & (j >= 0)
    e = np.stack([np.minimum(i, j)[keep], np.maximum(i, j)[keep]], 1)
    return np.unique(e, axis=0)


def normal_dot(nrm, a, b):
    x = np.asarray(nrm, np.float32).astype(np.float64)
    r = x[a, 0] * x[b, 0]
    r = r + x[a, 1] * x[b, 1]
    r = r + x[a, 2] * x[b, 2]
    return r


def root_index(p):
    z = np.asarray(p, np.float32)[:, 2].astype(np.float64)
    return int(np.argmax(z))  # the first of the maxima: Open3D's loop uses a strict >


def propagate(p, nrm, tree):
    """The flip bits: parity of the dot < 0 edges on the path from the root."""
    n = len(p)
    root = root_index(p)
    flip = np.zeros(n, bool)
    flip[root] = np.float32(nrm[root, 2]) < 0
    neg = normal_dot(nrm, tree[:, 0], tree[:, 1]) < 0 if len(tree) else np.zeros(0, bool)
    adj = [[] for _ in range(n)]
    for (a, b), s in zip(np.asarray(tree).tolist(), neg.tolist()):
        adj[a].append((b, s))
        adj[b].append((a, s))
    seen = np.zeros(n, bool)
    seen[root] = True
    stack = [root]
    while stack:
        u = stack.pop()
        for v, s in adj[u]:
            if not seen[v]:
                seen[v] = True
                flip[v] = flip[u] ^ s
                stack.append(v)
    assert seen.all(), "the tree spans the cloud"
    return flip


def orient(p, nrm, k, reverse_ties=False, d2=None, emst_edges=None):
    """dict(knn, emst, tree, flip, normals, outside): the rule on float32 points
    and float32 normals.  outside = EMST edges that are no kNN edge.  d2 /
    emst_edges: precomputed d2_dense(p) / emst(p) of the same points."""
    p = np.asarray(p, np.float32)
    nrm = np.asarray(nrm, np.float32)
    n = len(p)
    d2 = d2_dense(p) if d2 is None else d2
    knn = knn_lists(d2, k)
    E = emst(p, d2, reverse_ties) if emst_edges is None else np.asarray(emst_edges, np.int32)
    ke = knn_edges(knn)
    rg = np.unique(np.concatenate([ke, E.astype(np.int64)]), axis=0) if n > 1 else np.zeros((0, 2), np.int64)
    w = 1.0 - np.abs(normal_dot(nrm, rg[:, 0], rg[:, 1]))
    t = kruskal(n, rg[:, 0], rg[:, 1], w, reverse_ties)
    assert len(t) == max(n - 1, 0), "the Riemannian graph contains the EMST, so it is connected"
    tree = sort_edges(rg[t])
    flip = propagate(p, nrm, tree)
    out = nrm.copy()
    out[flip] = -out[flip]
    kset = set(map(tuple, ke.tolist()))
    outside = sum(1 for e in E.tolist() if tuple(e) not in kset)
    return {"knn": knn, "emst": E, "tree": tree, "flip": flip, "normals": out, "outside": outside}


def pca_normals(p, k):
    """Plain float64 PCA normals of the k nearest neighbours, rounded to
    float32 (fixture inputs only; their signs are whatever eigh returns)."""
    p = np.asarray(p, np.float32)
    knn = knn_lists(d2_dense(p), k)
    q = p.astype(np.float64)[knn]
    c = q - q.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c)
    _, v = np.linalg.eigh(cov)
    return v[:, :, 0].astype(np.float32)
