/*
 * o3dx.h — C-ABI of libo3dx.so, the MI355X (gfx950) point-cloud hot path behind
 * the open3dpypro drop-in (qinhy/Open3D-py-extension).
 *
 * The reference is pure Python; every hot-path call in it falls through to
 * Open3D 0.19's C++ CPU kernels via pybind11.  Each entry point below replaces
 * one of those calls; the replaced reference call site is cited per function.
 * The Python binding (ctypes) lives in open3dpypro/_native.py; INTEGRATION.md
 * shows the binding a maintainer would add.
 *
 * Conventions (all functions):
 *   - Plain pointers and sizes only.  "dev" = device (HBM) pointer, "host" =
 *     host pointer.  Points are (n,3) float32, row-major (AoS, 12 B / point).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     Work is enqueued on it; functions that return a host value (counts,
 *     bounds, transforms) synchronise that stream before returning.
 *   - The caller owns every buffer, including the scratch workspace
 *     (`ws`, `ws_bytes`, from the matching *_workspace_bytes query, 256-B
 *     aligned).  The library never allocates device memory, never frees
 *     caller memory and keeps no pointer after return.
 *   - Return 0 on success, a negative errno on failure:
 *       O3DX_EINVAL  bad argument (mirrors Open3D's LogError -> RuntimeError)
 *       O3DX_ENOMEM  workspace too small
 *       O3DX_EIO     HIP runtime error
 *       O3DX_ENOTSUP configuration outside this implementation's range
 *     o3dx_last_error() returns the thread-local message of the last failure.
 *   - Indices are int32 (Open3D uses int for point ids; n < 2^31).
 */
#ifndef O3DX_H
#define O3DX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define O3DX_ABI_VERSION 7

#define O3DX_OK 0
#define O3DX_EIO (-5)
#define O3DX_ENOMEM (-12)
#define O3DX_EINVAL (-22)
#define O3DX_ENOTSUP (-95)

/* search modes of estimate_normals / knn search
 * (KDTreeSearchParamKNN / Radius / Hybrid, reference PointCloud.py:68, test_mesh.py:18) */
#define O3DX_SEARCH_KNN 0
#define O3DX_SEARCH_RADIUS 1
#define O3DX_SEARCH_HYBRID 2

/* largest k served by the register top-k path (KNN k, HYBRID max_nn) */
#define O3DX_MAX_KNN 64

/* ICP reduction vector layout (o3dx_icp_accumulate):
 *   [0..20]  JTJ upper triangle, row-major (6x6)
 *   [21..26] JTr
 *   [27]     sum r^2         (point-to-plane residuals)
 *   [28]     correspondence count
 *   [29]     sum d^2         (squared correspondence distances, for inlier_rmse)
 *   [30..31] reserved (0)
 * (point-to-point estimation: its own layout in the same vector, "Point-to-point
 * ICP" below; [28] and [29] keep their meaning) */
#define O3DX_ICP_NSUMS 32
/* length of the ICP target descriptor (doubles) */
#define O3DX_ICP_DESC_LEN 24

/* ---------------------------------------------------------------- misc */
int o3dx_abi_version(void);
const char* o3dx_last_error(void);
/* fx sums (see o3dx_plane_moments) -> float64: k rows {lo, hi, q, 0} ->
 * out[k] = (hi * 2^32 + lo) * 2^q, correctly rounded.  Host only. */
int o3dx_fx_to_double(const int64_t* fx_host, int64_t k, double* out_host);

/* Kernel timing (measurement support, off by default): when enabled, the
 * library brackets its main kernel launches with hipEvents on the launch
 * stream; o3dx_kernel_timing() waits for the pending events and returns the
 * accumulated milliseconds and launch count of one kernel by name
 * ("voxel_assign", "normals_knn", "grid_build", "plane_count",
 * "icp_accumulate", ...).  Returns 0 if the name was seen, -1 otherwise.
 * Process-wide profiling switch (mutex-guarded event lists): the one piece of
 * state shared across threads; it adds event records, never changes results. */
void o3dx_set_kernel_timing(int enable);
/* Restrict timing to the comma-separated timer names ("" or NULL: all). */
void o3dx_kernel_timing_filter(const char* names_csv);
void o3dx_reset_kernel_timing(void);
int o3dx_kernel_timing(const char* name, double* total_ms, int64_t* launches);

/* Debug-only neighbour-search statistics: when enabled, every grid search
 * (normals, kNN, ICP) adds {queries, cells visited, candidate points, shells}
 * into device counters, and the KNN-normals levels count the queries they
 * hand on {tile -> wave form, wave form -> register top-k} and why the tile
 * gave up {box over LDS capacity, too few points within the shell-1 radius};
 * o3dx_search_stats copies those eight counters out (synchronises the device).
 * Enabling allocates a 64-byte device buffer — the only device allocation the
 * library ever makes; off by default.  Thread-local: the setting and buffer
 * belong to the calling host thread (one buffer per thread that enables it). */
int o3dx_set_search_stats(int enable);
int o3dx_search_stats(int64_t* out8_host);

/* Test hooks (parity evidence; no reference counterpart).
 *
 * o3dx_set_debug_neighbors: while buf_dev is non-null, every KNN-normals
 * kernel (voxel-table blocks, LDS tiles, wave form, register top-k) writes the
 * k neighbour ids it selected for output row r into buf_dev[r*k .. r*k+k) (in
 * the order it summed them; ids = the caller's point rows).  Only calls whose
 * k equals `k` and whose rows are < `rows` write.  NULL turns it off.  The
 * buffer is caller-owned; the library keeps the pointer until it is reset.
 * Thread-local: only launches made by the thread that set it write.
 *
 * o3dx_fast_eigen3x3: the device FastEigen3x3 (the normals kernels' solver)
 * on m covariances {xx,xy,xz,yy,yz,zz} (f64, dev) -> smallest-eigenvalue
 * eigenvectors (m,3) f64 (dev).  Asynchronous.
 *
 * o3dx_libm_probe: the device double-precision function the normals use
 * (fn 0 = acos, 1 = cos, 2 = sqrt) on n values (dev) -> out (dev).
 *
 * o3dx_normal_finish_check (additive to ABI 7): the normals kernels' finish,
 * covariance tail + FastEigen3x3, on m sets of nine raw moments {x, y, z, xx,
 * xy, xz, yy, yz, zz} (m,9) f64 (dev) of k >= 1 points each -> covariances
 * {xx,xy,xz,yy,yz,zz} (m,6) and eigenvectors (m,3), f64 (dev).  ref = 0 runs
 * the product formulation (selects, shared-divisor exact division), ref != 0
 * Open3D's text (an arm per case, a division per quotient); the two must
 * agree bit for bit.  Asynchronous. */
int o3dx_set_debug_neighbors(int32_t* buf_dev, int64_t rows, int k);
int o3dx_fast_eigen3x3(const double* cov_dev, int64_t m, double* out_dev, void* stream);
int o3dx_normal_finish_check(const double* mom9_dev, int64_t m, int k, int ref, double* cov6_out_dev,
                             double* vec3_out_dev, void* stream);
int o3dx_libm_probe(const double* x_dev, int64_t n, int fn, double* out_dev, void* stream);

/* ---------------------------------------------------------------- AABB
 * Replaces o3d.geometry.PointCloud.get_min_bound()/get_max_bound()
 * (reference PointCloud.py:145-146, :340).
 * minmax_host = {minx, miny, minz, maxx, maxy, maxz}; n == 0 gives zeros
 * (Open3D returns a zero vector for an empty cloud).  Synchronises. */
size_t o3dx_aabb_workspace_bytes(int64_t n);
int o3dx_aabb(const float* xyz_dev, int64_t n, double* minmax_host,
              void* ws, size_t ws_bytes, void* stream);
/* The same into a device double[6], asynchronous (no host wait): the
 * multi-GPU path all-reduces the bounds on the device before one read. */
int o3dx_aabb_device(const float* xyz_dev, int64_t n, double* minmax_dev,
                     void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- voxel
 * Replaces o3d PointCloud.voxel_down_sample_and_trace(voxel_size, min_bound,
 * max_bound, approximate_class=False) + idxmat.max(1) + _select_by_idx
 * (reference PointCloud.py:338-341, :361-362, :185-204; processors.py:427-430).
 *
 * key(p) = floor((p - min_bound) / voxel_size) per axis, computed in float64
 * exactly as Open3D does.  The representative of a voxel is the largest
 * original index in it (= idxmat.max(1)).  Output is in ascending original
 * index order (= _select_by_idx order):
 *   rep_idx_dev[0..m)          representative indices, ascending     (cap n)
 *   rep_xyz_dev[0..3m)         their coordinates (nullable)          (cap 3n)
 *   voxel_of_point_dev[0..n)   output row of each input point (nullable)
 *   cubic_id_dev[0..8m)        Open3D's (M,8) cubic-id matrix, -1 filled,
 *                              row r = voxel of rep_idx[r] (nullable, cap 8n)
 * min_bound_host / max_bound_host: NULL -> the cloud's AABB (device pass).
 * Errors (RuntimeError in Python, as Open3D): voxel_size <= 0;
 * voxel_size * INT_MAX < max extent ("voxel_size is too small.").
 * Synchronises (m is returned on the host). */
size_t o3dx_voxel_workspace_bytes(int64_t n);
int o3dx_voxel_down_sample(const float* xyz_dev, int64_t n,
                           const double* min_bound_host,
                           const double* max_bound_host, double voxel_size,
                           int32_t* rep_idx_dev, float* rep_xyz_dev,
                           int64_t* m_host, int32_t* voxel_of_point_dev,
                           int32_t* cubic_id_dev, void* ws, size_t ws_bytes,
                           void* stream);

/* Voxel down-sample that also keeps its voxel grid for a following
 * estimate_normals on the representatives (the pipeline
 * pcd.voxel_down_sample(vs).estimate_normals(), reference PointCloud.py:361,
 * :68).  o3dx_voxel_grid_cells(n, min, max, vs): the number of voxels nvox of
 * the dense voxel table for these bounds (host arithmetic), 0 when the grid
 * is too sparse to keep; o3dx_voxel_grid_capacity(n): the largest nvox any
 * call on n points keeps (a table buffer of that many voxels fits whatever
 * the bounds turn out to be).  o3dx_voxel_down_sample_grid: same outputs as
 * o3dx_voxel_down_sample (null bounds: the AABB, computed on the device),
 * plus, when nvox <= voxel_cells (the capacity of voxel_pts_dev),
 *   voxel_pts_dev[0..4 nvox)  per voxel (x, y, z, output row as int32 bits)
 *                             of its representative, row -1 when empty
 *   geom_host[12]             {min_bound xyz, voxel_size, nx, ny, nz, valid,
 *                              occupied 2^3-voxel cells, x-key offset,
 *                              build attempt (0: first), nvox}
 * valid = 0 when the table could not be kept (too sparse, larger than
 * voxel_cells, or points outside the bounds).  One host synchronisation for
 * m (two with null bounds). */
int64_t o3dx_voxel_grid_cells(int64_t n, const double* min_bound_host,
                              const double* max_bound_host, double voxel_size);
int64_t o3dx_voxel_grid_capacity(int64_t n);
int o3dx_voxel_down_sample_grid(const float* xyz_dev, int64_t n,
                                const double* min_bound_host,
                                const double* max_bound_host, double voxel_size,
                                int32_t* rep_idx_dev, float* rep_xyz_dev,
                                int64_t* m_host, int32_t* voxel_of_point_dev,
                                int32_t* cubic_id_dev, float* voxel_pts_dev,
                                int64_t voxel_cells, double* geom_host,
                                void* ws, size_t ws_bytes, void* stream);

/* Slab form (C4: one cloud spread over GPUs as voxel-aligned x-slabs,
 * open3dpypro.distributed.voxel_normals_slabs).  Keys are those of the GLOBAL
 * min_bound (so every voxel and representative is the single-GPU one); only
 * the x keys [kx0, kx1) are materialised.
 * o3dx_voxel_down_sample_window: o3dx_voxel_down_sample_grid restricted to
 * the window (every point must fall inside it; voxel_pts_dev nullable);
 * geom_host[0] is then the window's x origin and geom_host[9] = kx0.
 * o3dx_voxel_table_build: the voxel table (x, y, z, row) of n points holding
 * at most one point per voxel — a slab's own + halo representatives in their
 * global order — over the same window, plus geom_host, for
 * o3dx_estimate_normals_voxel.  Errors: a point outside the window, two
 * points in one voxel.  Synchronises. */
int o3dx_voxel_down_sample_window(const float* xyz_dev, int64_t n,
                                  const double* min_bound_host,
                                  const double* max_bound_host, double voxel_size,
                                  int64_t kx0, int64_t kx1, int32_t* rep_idx_dev,
                                  float* rep_xyz_dev, int64_t* m_host,
                                  float* voxel_pts_dev, int64_t voxel_cells,
                                  double* geom_host, void* ws, size_t ws_bytes,
                                  void* stream);
size_t o3dx_voxel_table_workspace_bytes(void);
int o3dx_voxel_table_build(const float* xyz_dev, int64_t n,
                           const double* min_bound_host,
                           const double* max_bound_host, double voxel_size,
                           int64_t kx0, int64_t kx1, float* voxel_pts_dev,
                           int64_t voxel_cells, double* geom_host, void* ws,
                           size_t ws_bytes, void* stream);
/* o3dx_voxel_table_build_deferred: the same table without the host wait.
 * Rows with a non-finite coordinate are skipped (padding rows of a
 * fixed-size halo exchange).  The error bits (1: a point outside the window,
 * 2: two points in one voxel) are OR-ed into status_dev[0] (int64, caller
 * zeroed) for the caller to check later; the occupancy is not measured
 * (geom_host[8] = -1), and o3dx_estimate_normals_voxel then runs the
 * voxel-table kernels without the occupancy test (their results do not
 * depend on it).  Multi-GPU slab step: replaces Python-side waits. */
int o3dx_voxel_table_build_deferred(const float* xyz_dev, int64_t n,
                                    const double* min_bound_host,
                                    const double* max_bound_host, double voxel_size,
                                    int64_t kx0, int64_t kx1, float* voxel_pts_dev,
                                    int64_t voxel_cells, double* geom_host,
                                    int64_t* status_dev, void* stream);

/* The slab step without host waits between the voxel window and the verdict
 * (ABI 6; open3dpypro.distributed.voxel_normals_slabs, the reference's
 * per-rank placement processors.py:206-207 scaled to one cloud over ranks).
 * o3dx_voxel_down_sample_window_deferred: o3dx_voxel_down_sample_window
 * (no table kept) whose counts stay on the device: counts_dev[3] (int64)
 * = {m, error bits, occupancy}; error bit 16 = the one-pass binning
 * overflowed (re-run the synchronous form), any other bit = points outside
 * the window.  rep_idx_dev / rep_xyz_dev hold m rows.
 * o3dx_slab_halo_pack: over the window's m reps (capacity cap rows): the
 * reps' global ids rg_out[i] = gidx_dev[rep_idx[i]] (int64), and, when
 * pcap > 0, send_dev (2 pcap, 4) float32 = the reps whose x key
 * floor((x - min_x) / voxel_size) is < k_lo_send (has_lo) in rows
 * [0, pcap), >= k_hi_send (has_hi) in rows [pcap, 2 pcap), each part in rep
 * order as (x, y, z, int32 bits of the global id), padded with NaN rows of
 * id INT32_MAX.  Workspace o3dx_slab_pack_workspace_bytes(cap).
 * o3dx_slab_halo_merge: the own reps and the received rows (na rows from the
 * lower neighbour then nb from the upper, each ascending in id, padding
 * last) merged into ascending global id: ux_dev (ux_rows >= cap + na + nb,
 * 3) float32, NaN past the union; own_pos_dev[i] = the union row of own rep
 * i; nu_dev[0] = the union size.
 * o3dx_slab_verdict: after the normals of the union rows (normals_union,
 * kd2_union from o3dx_estimate_normals_voxel): normals_own[i] = the own
 * reps' normals; info_dev[5] (int64) = {1 if some own rep's sqrt(kd2) >=
 * (t + halo)(1 - 1e-9), t its distance to the interior faces x_lo (has_lo)
 * / x_hi (has_hi); m; union size; the window's error bits; status_dev[0]}.
 * No host synchronisation in any of them. */
int o3dx_voxel_down_sample_window_deferred(const float* xyz_dev, int64_t n,
                                           const double* min_bound_host,
                                           const double* max_bound_host,
                                           double voxel_size, int64_t kx0, int64_t kx1,
                                           int32_t* rep_idx_dev, float* rep_xyz_dev,
                                           int64_t* counts_dev, void* ws,
                                           size_t ws_bytes, void* stream);
size_t o3dx_slab_pack_workspace_bytes(int64_t cap);
int o3dx_slab_halo_pack(const float* rep_xyz_dev, const int32_t* rep_idx_dev,
                        const int64_t* gidx_dev, const int64_t* counts_dev,
                        int64_t cap, double min_x, double voxel_size,
                        int64_t k_lo_send, int64_t k_hi_send, int has_lo, int has_hi,
                        int64_t* rg_out_dev, float* send_dev, int64_t pcap,
                        void* ws, size_t ws_bytes, void* stream);
int o3dx_slab_halo_merge(const float* rep_xyz_dev, const int64_t* rg_dev,
                         const int64_t* counts_dev, int64_t cap,
                         const float* recv_dev, int64_t na, int64_t nb,
                         float* ux_dev, int64_t ux_rows, int32_t* own_pos_dev,
                         int64_t* nu_dev, void* stream);
int o3dx_slab_verdict(const float* rep_xyz_dev, const int32_t* own_pos_dev,
                      const int64_t* counts_dev, int64_t cap,
                      const float* kd2_union_dev, const float* normals_union_dev,
                      double x_lo, double x_hi, int has_lo, int has_hi, double halo,
                      const int64_t* nu_dev, const int64_t* status_dev,
                      float* normals_own_dev, int64_t* info_dev, void* stream);

/* ---------------------------------------------------------------- normals
 * Replaces o3d PointCloud.estimate_normals(search_param,
 * fast_normal_computation=True) (reference PointCloud.py:68-73, used by
 * processors.py:243-249 CPUNormals): per point the neighbour set of
 * KDTreeFlann::Search (KNN k incl. the point itself / RADIUS d^2 < r^2 /
 * HYBRID nearest <= max_nn with d^2 < r^2), Open3D's raw-moment float64
 * covariance (identity if < 3 neighbours), FastEigen3x3 smallest eigenvector,
 * (0,0,1) if it is zero; if prior_normals_dev is given the result is flipped
 * to agree with it (Open3D's has_normal branch).
 * normals_out_dev: (n,3) float32.  KNN/HYBRID require k <= O3DX_MAX_KNN.
 * kth_d2_dev (nullable, KNN only): (n,) float32, per point an upper bound of
 * the squared distance of its k-th neighbour (>= the exact float64 value, to
 * a few float32 ulps) — what a spatially sharded caller needs to prove a halo
 * wide enough (open3dpypro.distributed.voxel_normals_slabs). */
size_t o3dx_normals_workspace_bytes(int64_t n);
int o3dx_estimate_normals(const float* xyz_dev, int64_t n, int mode, int knn,
                          double radius, const float* prior_normals_dev,
                          float* normals_out_dev, float* kth_d2_dev, void* ws,
                          size_t ws_bytes, void* stream);

/* estimate_normals of the m representatives of o3dx_voxel_down_sample_grid
 * (rep_xyz_dev, voxel_pts_dev, geom_host from that call): the search grid is
 * read off the voxel table (cells of b^3 voxels, b in 1..4 chosen from the
 * occupied 2^3-cell count) — or, for volumetric clouds, the table itself is
 * the search structure (4^3-voxel blocks staged in LDS) — instead of being
 * rebuilt by sorting; same neighbour sets and results as
 * o3dx_estimate_normals(rep_xyz_dev, m, ...).
 * Workspace: o3dx_normals_workspace_bytes(m).  No host synchronisation. */
int o3dx_estimate_normals_voxel(const double* geom_host,
                                const float* voxel_pts_dev,
                                const float* rep_xyz_dev, int64_t m, int mode,
                                int knn, double radius,
                                const float* prior_normals_dev,
                                float* normals_out_dev, float* kth_d2_dev,
                                void* ws, size_t ws_bytes, void* stream);

/* The pipeline pcd.voxel_down_sample(vs).estimate_normals(KNN(knn))
 * (reference PointCloud.py:361, :68) in one call: the outputs of
 * o3dx_voxel_down_sample_grid (rep_idx, rep_xyz, m, voxel_pts, geom) plus
 * normals_out_dev[0..3m) = o3dx_estimate_normals_voxel on the
 * representatives, bit for bit.  The normals kernels over the kept table are
 * queued behind the voxel kernels before m is read back (one host
 * synchronisation for the whole pipeline besides the bounds); if the table
 * path turns out not to apply (sparse cloud, m < knn) the normals are
 * recomputed by the general path.  ws: o3dx_voxel_workspace_bytes(n);
 * nws: o3dx_normals_workspace_bytes(n); rep_xyz_dev, normals_out_dev cap n. */
int o3dx_voxel_down_sample_normals(const float* xyz_dev, int64_t n,
                                   const double* min_bound_host,
                                   const double* max_bound_host, double voxel_size,
                                   int knn, int32_t* rep_idx_dev, float* rep_xyz_dev,
                                   float* normals_out_dev, int64_t* m_host,
                                   float* voxel_pts_dev, int64_t voxel_cells,
                                   double* geom_host, void* ws, size_t ws_bytes,
                                   void* nws, size_t nws_bytes, void* stream);

/* ---------------------------------------------------------------- kNN search
 * Batched form of KDTreeFlann.search_knn_vector_3d / search_hybrid_vector_3d
 * (reference PointCloud.py:148-163).  For each query q: up to K = knn (KNN)
 * or max_nn (HYBRID) nearest points of `xyz`, sorted by squared distance
 * (float64, computed as nanoflann does).  Outputs, row-major (nq, K):
 *   idx_out_dev (-1 padded), d2_out_dev (nullable, +inf padded),
 *   count_out_dev (nq). */
size_t o3dx_knn_workspace_bytes(int64_t n);
int o3dx_knn_search(const float* xyz_dev, int64_t n, const float* queries_dev,
                    int64_t nq, int mode, int knn, double radius,
                    int32_t* idx_out_dev, double* d2_out_dev,
                    int32_t* count_out_dev, void* ws, size_t ws_bytes,
                    void* stream);

/* ---------------------------------------------------------------- RANSAC
 * Replaces o3d PointCloud.segment_plane(distance_threshold, ransac_n,
 * num_iterations, probability=0.99999999) (reference PointCloud.py:75-77,
 * processors.py:637-638, seg_planes PointCloud.py:941-985).
 *
 * o3dx_ransac_samples: Open3D's RandomSampler — per iteration `ransac_n`
 *   distinct indices, each mt19937(seed)() % n, duplicates re-drawn.  Host only.
 * o3dx_segment_plane: hypotheses from `samples_host` (iters x ransac_n),
 *   ComputeTrianglePlane (n==3) / GetPlaneFromPoints, exact inlier counts
 *   (|n.p+d| < thr in float64), Open3D's sequential selection rule (fitness,
 *   then Sigma|d|/sqrt(cnt), early break at log(1-p)/log(1-fitness^n)),
 *   final inlier scan with the winning hypothesis and the least-squares refit.
 *   inliers_out_dev: ascending indices (cap n); plane_host: {a,b,c,d}.
 * Errors: probability not in (0,1], ransac_n < 3, n < ransac_n. */
int o3dx_ransac_samples(int64_t n, int ransac_n, int num_iterations,
                        uint64_t seed, int32_t* samples_host);
size_t o3dx_segment_plane_workspace_bytes(int64_t n, int num_iterations);
int o3dx_segment_plane(const float* xyz_dev, int64_t n,
                       double distance_threshold, int ransac_n,
                       int num_iterations, double probability,
                       const int32_t* samples_host, double* plane_host,
                       int32_t* inliers_out_dev, int64_t* n_inliers_host,
                       void* ws, size_t ws_bytes, void* stream);

/* Building blocks of o3dx_segment_plane, exposed for point-sharded multi-GPU
 * use (counts/sums are all-reduced between the calls).
 * o3dx_plane_from_points: host-only plane fit of `k` points (ComputeTrianglePlane
 *   for k==3 else GetPlaneFromPoints); zero plane if degenerate.
 * o3dx_plane_count: exact inlier count of each hypothesis (counts_host[h]).
 * o3dx_plane_abs_sum: Sigma |n.p+d| over inliers for the hypotheses listed in
 *   which_host (sums_host[j] for which_host[j]).
 * o3dx_ransac_select: Open3D's sequential selection replay on host; returns the
 *   winning hypothesis index (or -1). needs sums for count ties (NaN else).
 * o3dx_plane_inliers: ascending indices with |n.p+d| < thr (float64).
 * o3dx_plane_moments: sums over idx of {x,y,z} (pass 1, centroid NULL) or of
 *   centred {xx,xy,xz,yy,yz,zz} (pass 2), for GetPlaneFromPoints.
 *   absmax_host (nullable: the selected points' own): |x|,|y|,|z| bounds of
 *   the cloud, which fix the sums' fx quantum (below) — a sharded cloud
 *   passes the global bounds on every rank.
 * Sums of float terms here and in o3dx_icp_accumulate are "fx" sums: every
 *   term is rounded to an integer multiple of 2^q (q from a bound of the
 *   terms every rank derives alike) and the integers are added, so the sum
 *   does not depend on how the points are split over blocks or GPUs.
 *   fx_out_host (nullable) receives one row {lo, hi, q, 0} (int64) per sum:
 *   value = (hi * 2^32 + lo) * 2^q.  Rows of the same sum on several ranks
 *   add digit-wise (int64), then o3dx_fx_to_double rounds once. 
 * o3dx_plane_from_moments: host-only GetPlaneFromPoints from those sums. */
int o3dx_plane_from_points(const double* pts_host, int k, double* plane_host);
/* ComputeTrianglePlane / GetPlaneFromPoints of H hypotheses at once: coords
 * (H x ransac_n x 3 float64, host) -> planes (H x 4, host; zero = degenerate). */
int o3dx_planes_from_samples(const double* coords_host, int num_hypotheses,
                             int ransac_n, double* planes_host);
size_t o3dx_plane_count_workspace_bytes(int64_t n, int num_hypotheses);
int o3dx_plane_count(const float* xyz_dev, int64_t n, const double* planes_host,
                     int num_hypotheses, double distance_threshold,
                     int64_t* counts_host, void* ws, size_t ws_bytes,
                     void* stream);
/* Upper bounds of the inlier counts (counts_host[h] >= the exact count;
 * degenerate hypotheses -1): the float32 distance against the largest float32
 * window edge, no float64 re-decision.  absmax_host (nullable: the cloud's
 * own): |x|,|y|,|z| bounds of the cloud.  Paired with o3dx_ransac_needed, a
 * selection counts exactly only the hypotheses Open3D's replay consults. */
int o3dx_plane_count_upper(const float* xyz_dev, int64_t n, const double* planes_host,
                           int num_hypotheses, double distance_threshold,
                           const double* absmax_host, int64_t* counts_host, void* ws,
                           size_t ws_bytes, void* stream);
/* counts_host: exact counts where known_host[h] != 0, upper bounds elsewhere.
 * out_host (capacity num_hypotheses) receives the unknown hypotheses that
 * Open3D's selection replay on these values consults (records and ties,
 * ascending); *n_out == 0 means the selection (o3dx_ransac_tied /
 * o3dx_ransac_select on these values) equals the one on exact counts. */
int o3dx_ransac_needed(const int64_t* counts_host, const uint8_t* known_host,
                       const double* planes_host, int num_hypotheses, int64_t n,
                       int ransac_n, double probability, int32_t* out_host,
                       int32_t* n_out);
int o3dx_plane_abs_sum(const float* xyz_dev, int64_t n,
                       const double* planes_host, const int32_t* which_host,
                       int num_which, double distance_threshold,
                       double* sums_host, int64_t* fx_out_host, void* ws,
                       size_t ws_bytes, void* stream);
/* The hypotheses whose Sigma|d| Open3D's selection can consult (equal-count
 * ties at a running maximum, with its early break replayed on the counts),
 * ascending, into out_host (capacity num_hypotheses); *n_out = their number. */
int o3dx_ransac_tied(const int64_t* counts_host, const double* planes_host,
                     int num_hypotheses, int64_t n, int ransac_n,
                     double probability, int32_t* out_host, int32_t* n_out);
int o3dx_ransac_select(const int64_t* counts_host, const double* sums_host,
                       const double* planes_host, int num_hypotheses,
                       int64_t n, int ransac_n, double probability);
/* The early-stop point the three replays above set at a new best fitness:
 * 0 for fitness >= 1; num_hypotheses (no early stop) when the quotient
 * log(1 - probability) / log(1 - fitness^ransac_n) is not >= 0 (-inf or NaN
 * once fitness^ransac_n < 2^-53); else the quotient, capped at
 * num_hypotheses, truncated.  Host-only. */
int64_t o3dx_ransac_break_iteration(double fitness, int ransac_n, double probability,
                                    int num_hypotheses);
int o3dx_plane_inliers(const float* xyz_dev, int64_t n, const double* plane_host,
                       double distance_threshold, int32_t* idx_out_dev,
                       int64_t* count_host, void* ws, size_t ws_bytes,
                       void* stream);
/* Plane selection / distance (PointCloudSelections.get_index_by_plane,
 * select_by_plane, distance2plane — reference PointCloud.py:278-290, 400-404;
 * the seg_planes / remove_plane_outlier rounds, :406-409, :941-985).
 * s = ((x*a + y*b) + z*c + d) / sqrt(a*a + b*b + c*c) in float64, unfused (the
 * order of numpy's (p*abc).sum(1) + d).  dist_out_dev (optional): s per point.
 * idx_out_dev (optional): ascending indices with |s| < hi (band == 0) or
 * lo < s < hi (band == 1), complemented when invert != 0; count_host gets
 * their number.  Workspace only needed with idx_out_dev. */
size_t o3dx_plane_select_workspace_bytes(int64_t n);
int o3dx_plane_select(const float* xyz_dev, int64_t n, const double* plane_host,
                      int band, double lo, double hi, int invert,
                      double* dist_out_dev, int32_t* idx_out_dev,
                      int64_t* count_host, void* ws, size_t ws_bytes,
                      void* stream);
/* The same on float64 coordinates (ABI 3): a cloud built from float64 host
 * data keeps the caller's exact values, and the reference evaluates the
 * distance on them (PointCloud.py:400-404 on get_points(), float64). */
int o3dx_plane_select_f64(const double* xyz_dev, int64_t n, const double* plane_host,
                          int band, double lo, double hi, int invert,
                          double* dist_out_dev, int32_t* idx_out_dev,
                          int64_t* count_host, void* ws, size_t ws_bytes,
                          void* stream);
size_t o3dx_plane_moments_workspace_bytes(int64_t count);
int o3dx_plane_moments(const float* xyz_dev, const int32_t* idx_dev,
                       int64_t count, const double* centroid_host,
                       const double* absmax_host, double* sums_host,
                       int64_t* fx_out_host, void* ws, size_t ws_bytes,
                       void* stream);
int o3dx_plane_from_moments(const double* sum_xyz_host, int64_t count,
                            const double* centred_host, double* plane_host);

/* ---------------------------------------------------------------- ICP
 * Point-to-plane ICP (north-star op; absent from the reference — attached as
 * PointCloud.registration_icp / Processors.ICP).  Semantics of Open3D's
 * registration_icp + TransformationEstimationPointToPlane: correspondences =
 * target nearest neighbour of T*src within max_correspondence_distance
 * (d^2 < r^2), r = (vs - vt).nt, J = [vs x nt ; nt], solve JTJ x = -JTr,
 * update = Rz(x2) Ry(x1) Rx(x0) | x[3..5], T <- update * T.
 *
 * o3dx_icp_target_build: builds the persistent target structure (spatial grid
 *   of target points + normals) inside `target_ws`; desc_host
 *   (O3DX_ICP_DESC_LEN doubles) receives its descriptor, to be passed back to
 *   o3dx_icp_accumulate / o3dx_icp_register.
 * o3dx_spatial_sort: (n,4) float32 copy of a cloud in a compact spatial order
 *   (grid cells of ~target_occ points, 8x8x8 blocks of cells, Morton order
 *   inside a block), w = bits of the original int32 index.  ICP sources are
 *   passed in this layout (src_sorted4 = 1) so that 64 consecutive queries
 *   form a compact patch (one LDS tile of target points); results are
 *   reported by original index.
 * o3dx_icp_accumulate: one pass over the source: transform by T_host
 *   (row-major 4x4, float64), 1-NN, residual/Jacobian, exact fx sums
 *   (o3dx_plane_moments note) into sums_host[O3DX_ICP_NSUMS] and, when
 *   fx_out_host is given, their rows (O3DX_ICP_NSUMS x 4 int64).
 *   src_absmax_host (nullable: this source's own): |x|,|y|,|z| bounds of the
 *   WHOLE source (a sharded source passes the global ones), which with T and
 *   the distance fix the fx quanta.  corr_out_dev (nullable, 2*ns int32
 *   pairs (i,j)) + ncorr_host receive the correspondence set.
 * o3dx_icp_solve_point_to_plane: host-only 6x6 LDLT solve of the summed
 *   system -> update_host (4x4 row-major); returns 1 if solved, 0 if singular
 *   (identity update, as Open3D).
 * o3dx_registration_icp_point_to_plane: the whole Open3D loop on one device
 *   (ws sized by o3dx_registration_icp_workspace_bytes; sorts the source once).
 * o3dx_icp_register (ABI 4): the same loop on a built target (desc_host) and a
 *   source as o3dx_icp_accumulate takes it (ws sized by
 *   o3dx_icp_accumulate_workspace_bytes): every iteration — the fused
 *   correspondence + moments pass, the solve, T <- update * T and Open3D's
 *   convergence test — runs on the device, the host waits once.  T is the
 *   same bits as a host loop of o3dx_icp_accumulate + o3dx_icp_update.
 */
size_t o3dx_icp_target_workspace_bytes(int64_t nt);
int o3dx_icp_target_build(const float* tgt_dev, const float* tgt_normals_dev,
                          int64_t nt, double max_correspondence_distance,
                          void* target_ws, size_t target_ws_bytes,
                          double* desc_host, void* stream);
size_t o3dx_icp_accumulate_workspace_bytes(int64_t ns);
int o3dx_icp_accumulate(const float* src_dev, int64_t ns, int src_sorted4,
                        const void* target_ws, const double* desc_host,
                        const double* T_host, double max_correspondence_distance,
                        const double* src_absmax_host, double* sums_host,
                        int64_t* fx_out_host, int32_t* corr_out_dev,
                        int64_t* ncorr_host, void* ws, size_t ws_bytes,
                        void* stream);
int o3dx_icp_solve_point_to_plane(const double* sums_host, double* update_host);
/* One ICP step on the host: solve the summed system and T <- update * T
 * (T_host row-major 4x4, in place), in the same float64 order as the
 * library's own registration loop; returns 1 if solved, 0 if singular. */
int o3dx_icp_update(const double* sums_host, double* T_host);
size_t o3dx_spatial_sort_workspace_bytes(int64_t n);
int o3dx_spatial_sort(const float* xyz_dev, int64_t n, double target_occ,
                      float* sorted4_dev, void* ws, size_t ws_bytes,
                      void* stream);
/* o3dx_spatial_sort_bounds (ABI 7, added): o3dx_spatial_sort that also
 * returns absmax_host[3] = the cloud's |x|,|y|,|z| bounds (from the bounds
 * the sort's grid already measures; the same values o3dx_icp_accumulate /
 * o3dx_icp_register would measure on the sorted copy), so the ICP call that
 * follows takes them as src_absmax_host and skips its own pass + host wait. */
int o3dx_spatial_sort_bounds(const float* xyz_dev, int64_t n, double target_occ,
                             float* sorted4_dev, double* absmax_host, void* ws,
                             size_t ws_bytes, void* stream);
int o3dx_icp_register(const float* src_dev, int64_t ns, int src_sorted4,
                      const void* target_ws, const double* desc_host,
                      const double* init_host, int max_iteration,
                      double relative_fitness, double relative_rmse,
                      double max_correspondence_distance,
                      const double* src_absmax_host, double* T_out_host,
                      double* fitness_host, double* inlier_rmse_host,
                      int32_t* corr_out_dev, int64_t* ncorr_host, void* ws,
                      size_t ws_bytes, void* stream);
size_t o3dx_registration_icp_workspace_bytes(int64_t ns);
int o3dx_registration_icp_point_to_plane(
    const float* src_dev, int64_t ns, const float* tgt_dev,
    const float* tgt_normals_dev, int64_t nt,
    double max_correspondence_distance, const double* init_host,
    int max_iteration, double relative_fitness, double relative_rmse,
    double* T_out_host, double* fitness_host, double* inlier_rmse_host,
    int32_t* corr_out_dev, int64_t* ncorr_host, void* target_ws,
    size_t target_ws_bytes, void* ws, size_t ws_bytes, void* stream);

/* Point-to-point ICP (additive to ABI 7): Open3D's registration_icp with
 * TransformationEstimationPointToPoint(with_scaling), its default estimation.
 * The loop, the correspondences and the convergence test are those above;
 * the update is Eigen::umeyama(P, Q, with_scaling) of the matched, already
 * transformed source points P and their target points Q: [cR | t], R = U S
 * V^T of the covariance (1/n) sum (q - qm)(p - pm)^T, S = diag(1, 1, +-1),
 * c = 1 or (s . diag S) / var(p), t = qm - c R pm.  It needs no target
 * normals.  `estimation` is one of the constants below (anything else:
 * O3DX_EINVAL, before any device call).
 *
 * Point-to-point sums (sums_host[O3DX_ICP_NSUMS]): the moments are taken
 * about a fixed anchor a, the target grid's origin (a float64 target's frame
 * origin), p' = p - a and q' = q - a in float64, so that a cloud far from the
 * coordinate origin loses nothing to cancellation:
 *   [0..8]   sum q'_a p'_b, row-major (3x3)
 *   [9..11]  sum p'
 *   [12..14] sum q'
 *   [15]     sum |p'|^2
 *   [16..18] the anchor a itself (set by the library; its fx rows are 0)
 *   [28]     correspondence count, [29] sum d^2 (as above); all others 0
 * The fx quanta follow from |q'| <= D (the target grid box's diagonal plus
 * its slack) and |p'| <= D + max_correspondence_distance, so they depend on
 * neither T nor the clouds' offset.  o3dx_icp_accumulate_est returns this
 * estimation's fx rows with the low digits' carry moved up (lo < 2^32), so
 * the rows themselves, not only their values, are the same for any order of
 * the source.
 *
 * o3dx_icp_target_build_points[_f64]: a target without normals (workspace as
 *   o3dx_icp_target_build[_f64]).  The point-to-plane entries refuse its
 *   descriptor (O3DX_EINVAL); point-to-point takes either kind of target.
 * o3dx_icp_accumulate_est, o3dx_icp_register_est[_f64],
 *   o3dx_registration_icp_est[_f64]: the entries above with the estimation
 *   (and with_scaling); tgt_normals_dev may be NULL for point-to-point.
 * o3dx_icp_solve_point_to_point / o3dx_icp_update_est: host only, the solve
 *   the device loop runs (the same bits); 1 if solved, 0 for the identity
 *   update (no correspondences, or a non-finite result such as with_scaling
 *   on a source of zero spread). */
#define O3DX_ICP_POINT_TO_PLANE 0
#define O3DX_ICP_POINT_TO_POINT 1
int o3dx_icp_target_build_points(const float* tgt_dev, int64_t nt,
                                 double max_correspondence_distance,
                                 void* target_ws, size_t target_ws_bytes,
                                 double* desc_host, void* stream);
int o3dx_icp_accumulate_est(const float* src_dev, int64_t ns, int src_sorted4,
                            const void* target_ws, const double* desc_host,
                            const double* T_host,
                            double max_correspondence_distance,
                            const double* src_absmax_host, double* sums_host,
                            int64_t* fx_out_host, int32_t* corr_out_dev,
                            int64_t* ncorr_host, int estimation, void* ws,
                            size_t ws_bytes, void* stream);
int o3dx_icp_register_est(const float* src_dev, int64_t ns, int src_sorted4,
                          const void* target_ws, const double* desc_host,
                          const double* init_host, int max_iteration,
                          double relative_fitness, double relative_rmse,
                          double max_correspondence_distance,
                          const double* src_absmax_host, double* T_out_host,
                          double* fitness_host, double* inlier_rmse_host,
                          int32_t* corr_out_dev, int64_t* ncorr_host,
                          int estimation, int with_scaling, void* ws,
                          size_t ws_bytes, void* stream);
int o3dx_registration_icp_est(
    const float* src_dev, int64_t ns, const float* tgt_dev,
    const float* tgt_normals_dev, int64_t nt,
    double max_correspondence_distance, const double* init_host,
    int max_iteration, double relative_fitness, double relative_rmse,
    double* T_out_host, double* fitness_host, double* inlier_rmse_host,
    int32_t* corr_out_dev, int64_t* ncorr_host, int estimation,
    int with_scaling, void* target_ws, size_t target_ws_bytes, void* ws,
    size_t ws_bytes, void* stream);
int o3dx_icp_solve_point_to_point(const double* sums_host, int with_scaling,
                                  double* update_host);
int o3dx_icp_update_est(const double* sums_host, int estimation,
                        int with_scaling, double* T_host);
int o3dx_icp_target_build_points_f64(const double* tgt_dev, int64_t nt,
                                     double max_correspondence_distance,
                                     void* target_ws, size_t target_ws_bytes,
                                     double* desc_host, void* stream);
int o3dx_icp_register_est_f64(const double* src_dev, int64_t ns, int src_sorted4,
                              const void* target_ws, const double* desc_host,
                              const double* init_host, int max_iteration,
                              double relative_fitness, double relative_rmse,
                              double max_correspondence_distance,
                              const double* src_absmax_host, double* T_out_host,
                              double* fitness_host, double* inlier_rmse_host,
                              int32_t* corr_out_dev, int64_t* ncorr_host,
                              int estimation, int with_scaling, void* ws,
                              size_t ws_bytes, void* stream);
int o3dx_registration_icp_est_f64(
    const double* src_dev, int64_t ns, const double* tgt_dev,
    const float* tgt_normals_dev, int64_t nt,
    double max_correspondence_distance, const double* init_host,
    int max_iteration, double relative_fitness, double relative_rmse,
    double* T_out_host, double* fitness_host, double* inlier_rmse_host,
    int32_t* corr_out_dev, int64_t* ncorr_host, int estimation,
    int with_scaling, void* target_ws, size_t target_ws_bytes, void* ws,
    size_t ws_bytes, void* stream);

/* Sharded ICP device loop (ABI 7; distributed.registration_icp_sharded, the
 * north star's "6x6 JTJ RCCL all-reduce", SURVEY 8(e) ICP row).  Each rank
 * holds a share of the source (src as o3dx_icp_register takes it) and the
 * target (replicated, or the window its share can reach) and queues per
 * iteration it = 0 .. max_iteration, with no host wait:
 *   o3dx_icp_shard_step    the rank's fused match + fx-moment step (skip proof
 *                          included; use_prior = 0 on the first step and
 *                          after a resume) and its digit sums -> digits_dev
 *                          (2 x 32 int64, device);
 *   (caller)               SUM all-reduce of digits_dev over the ranks;
 *   o3dx_icp_shard_finish  sums, fitness / rmse over n_total (the GLOBAL
 *                          source count), Open3D's convergence test, the 6x6
 *                          solve and T <- update * T: identical on every rank.
 * src_absmax_host (begin) must be the GLOBAL source bounds (fx quanta): T is
 * then o3dx_icp_register's on the whole source to the bit.  win_dev (nullable,
 * device, world rows {box min xyz, box max xyz, window lo, window hi}): the
 * finish stops the loop when the new T needs target rows outside some rank's
 * window (info[2] of o3dx_icp_shard_state); the caller refetches the windows
 * and calls o3dx_icp_shard_resume, then continues from it = info[1].  widen
 * (step and finish alike): the window's cover beyond the correspondence
 * radius; a grid whose skip-proof ball extension (0.1 cell) exceeds it
 * searches in full (+inf: replicated target, no cap).  ws is
 * sized by o3dx_icp_accumulate_workspace_bytes(ns) and carries the state
 * between the calls.  float32 clouds. */
int o3dx_icp_shard_begin(const double* init_host, const double* src_absmax_host,
                         double max_correspondence_distance, int64_t ns,
                         void* ws, size_t ws_bytes, void* stream);
int o3dx_icp_shard_step(const float* src_dev, int64_t ns, int src_sorted4,
                        const void* target_ws, const double* desc_host,
                        double max_correspondence_distance, int use_prior,
                        double widen, int64_t* digits_dev, void* ws, size_t ws_bytes,
                        void* stream);
int o3dx_icp_shard_finish(const int64_t* digits_dev, int64_t n_total, int it,
                          int max_iteration, double relative_fitness,
                          double relative_rmse,
                          double max_correspondence_distance,
                          const double* desc_host, const double* win_dev,
                          int world, double widen, int64_t ns, void* ws,
                          size_t ws_bytes, void* stream);
int o3dx_icp_shard_state(int64_t ns, void* ws, size_t ws_bytes,
                         double* T_out_host, double* fitness_host,
                         double* inlier_rmse_host, int32_t* info3_host,
                         void* stream);
int o3dx_icp_shard_resume(int64_t ns, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- PCD IO
 * o3dx_pcd_unpack: decode PCD fields on the device (replaces the host-side
 * field decoding of o3d.io.read_point_cloud behind PointCloudBase.read_pcd,
 * reference PointCloud.py:165-166).  data_dev holds the raw DATA bytes
 * (binary: n records; binary_compressed: the decompressed column blocks).
 * Field j (nfields <= 16) of point i is read at
 *   data_dev + src_off_host[j] + i * src_stride_host[j]   (no alignment needed)
 * as types_host[j], converted to float32 and stored at
 *   dst_dev_host[j] + i * dst_stride_host[j]   (floats).
 * O3DX_PCD_RGB reads a packed 0x00RRGGBB (F4 or U4 bits) and stores r, g, b
 * (3 consecutive floats, each /255).  Enqueues only. */
#define O3DX_PCD_F4 1
#define O3DX_PCD_F8 2
#define O3DX_PCD_U1 3
#define O3DX_PCD_U2 4
#define O3DX_PCD_U4 5
#define O3DX_PCD_I1 6
#define O3DX_PCD_I2 7
#define O3DX_PCD_I4 8
#define O3DX_PCD_RGB 9
/* o3dx_lzf_decompress (host): liblzf stream -> dst_host; returns the
 * decompressed length, or a negative error for a corrupt stream. */
int64_t o3dx_lzf_decompress(const uint8_t* src_host, int64_t n, uint8_t* dst_host, int64_t dst_len);
int o3dx_pcd_unpack(const uint8_t* data_dev, int64_t n, int nfields, const int32_t* types_host,
                    const int64_t* src_off_host, const int64_t* src_stride_host,
                    float* const* dst_dev_host, const int64_t* dst_stride_host, void* stream);

/* ------------------------------------------------------- one-query search
 * (ABI 5) One KDTreeFlann query of any size (reference PointCloud.py:148-163:
 * get_points_by_knn asks for up to 10^6 neighbours, get_points_radius for
 * every point within a radius): mode O3DX_SEARCH_KNN (the knn nearest),
 * RADIUS (every point with d^2 < radius^2) or HYBRID (the knn nearest of
 * those).  d^2 in float64 in nanoflann's order on the cloud's coordinates
 * (xyz_f64: (n,3) float64, else float32); results sorted by (d^2, index).
 * idx_out_dev / d2_out_dev (nullable) receive the first min(count, cap);
 * count_host the full count.  Synchronises the stream. */
size_t o3dx_search_one_workspace_bytes(int64_t n);
int o3dx_search_one(const void* xyz_dev, int xyz_f64, int64_t n, const double* query_host, int mode, int64_t knn,
                    double radius, int32_t* idx_out_dev, double* d2_out_dev, int64_t cap, int64_t* count_host,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------- float64 boundary
 * (ABI 5) The hot-path calls on (n,3) float64 clouds, computed on the
 * caller's float64 values exactly as Open3D computes them on its float64
 * storage (set_points keeps a float64 Vector3dVector, reference
 * PointCloud.py:99-102; LAS / E57 scans at georeferenced offsets,
 * :535-547, :646-687, are not float32-representable).  Same arguments,
 * errors and workspace rules as the float32 entry points named; the
 * PointCloud front end takes these only for clouds float32 cannot hold.
 *
 * o3dx_aabb_f64: get_min_bound / get_max_bound (PointCloud.py:145-146).
 * o3dx_voxel_down_sample_f64: voxel_down_sample_and_trace + idxmat.max(1)
 *   (PointCloud.py:338-341): keys floor((p - min) / vs) in float64;
 *   rep_xyz_dev (nullable) receives the representatives' float64 coordinates;
 *   the trace outputs as o3dx_voxel_down_sample.  ENOTSUP beyond 2^22 voxels
 *   per axis.
 * o3dx_estimate_normals_f64: estimate_normals (PointCloud.py:68-73): kNN /
 *   hybrid / radius sets by float64 (d^2, index), Open3D's raw-moment
 *   covariance summed in that order (float64, unfused) and FastEigen3x3;
 *   normals out float32.
 * o3dx_knn_search_f64: KDTreeFlann.search_knn / hybrid (PointCloud.py:148-163)
 *   for float64 points and queries.
 * o3dx_plane_count_f64 / o3dx_segment_plane_f64: exact per-hypothesis counts
 *   |(a x + c z) + (b y + d)| < thr on the float64 coordinates, and
 *   segment_plane (PointCloud.py:75-77) over them.
 * o3dx_icp_target_build_f64 / o3dx_spatial_sort_f64 (sorted4: (n,4) float64,
 *   w = original index) / o3dx_icp_register_f64 /
 *   o3dx_registration_icp_point_to_plane_f64: point-to-plane ICP with float64
 *   sources and targets (float32 target normals); a float64 target descriptor
 *   is refused by the float32 ICP entries and vice versa. */
size_t o3dx_aabb_f64_workspace_bytes(int64_t n);
int o3dx_aabb_f64(const double* xyz_dev, int64_t n, double* minmax_host, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_voxel_f64_workspace_bytes(int64_t n);
int o3dx_voxel_down_sample_f64(const double* xyz_dev, int64_t n, const double* min_bound_host,
                               const double* max_bound_host, double voxel_size, int32_t* rep_idx_dev,
                               double* rep_xyz_dev, int64_t* m_host, int32_t* voxel_of_point_dev,
                               int32_t* cubic_id_dev, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_normals_f64_workspace_bytes(int64_t n);
int o3dx_estimate_normals_f64(const double* xyz_dev, int64_t n, int mode, int knn, double radius,
                              const float* prior_normals_dev, float* normals_out_dev, float* kd2_out_dev,
                              void* ws, size_t ws_bytes, void* stream);
size_t o3dx_knn_f64_workspace_bytes(int64_t n);
int o3dx_knn_search_f64(const double* xyz_dev, int64_t n, const double* queries_dev, int64_t nq, int mode,
                        int knn, double radius, int32_t* idx_out_dev, double* d2_out_dev, int32_t* cnt_out_dev,
                        void* ws, size_t ws_bytes, void* stream);
int o3dx_plane_count_f64(const double* xyz_dev, int64_t n, const double* planes_host, int H, double thr,
                         int64_t* counts_host, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_segment_plane_f64_workspace_bytes(int64_t n, int num_iterations);
int o3dx_segment_plane_f64(const double* xyz_dev, int64_t n, double distance_threshold, int ransac_n,
                           int num_iterations, double probability, const int32_t* samples_host,
                           double* plane_host, int32_t* inliers_out_dev, int64_t* n_inliers_host, void* ws,
                           size_t ws_bytes, void* stream);
size_t o3dx_icp_target_f64_workspace_bytes(int64_t nt);
int o3dx_icp_target_build_f64(const double* tgt_dev, const float* tgt_normals_dev, int64_t nt,
                              double max_correspondence_distance, void* target_ws, size_t target_ws_bytes,
                              double* desc_host, void* stream);
size_t o3dx_spatial_sort_f64_workspace_bytes(int64_t n);
int o3dx_spatial_sort_f64(const double* xyz_dev, int64_t n, double target_occ, double* sorted4_dev, void* ws,
                          size_t ws_bytes, void* stream);
int o3dx_icp_register_f64(const double* src_dev, int64_t ns, int src_sorted4, const void* target_ws,
                          const double* desc_host, const double* init_host, int max_iteration,
                          double relative_fitness, double relative_rmse, double max_correspondence_distance,
                          const double* src_absmax_host, double* T_out_host, double* fitness_host,
                          double* inlier_rmse_host, int32_t* corr_out_dev, int64_t* ncorr_host, void* ws,
                          size_t ws_bytes, void* stream);
size_t o3dx_registration_icp_f64_workspace_bytes(int64_t ns);
int o3dx_registration_icp_point_to_plane_f64(
    const double* src_dev, int64_t ns, const double* tgt_dev, const float* tgt_normals_dev, int64_t nt,
    double max_correspondence_distance, const double* init_host, int max_iteration, double relative_fitness,
    double relative_rmse, double* T_out_host, double* fitness_host, double* inlier_rmse_host,
    int32_t* corr_out_dev, int64_t* ncorr_host, void* target_ws, size_t target_ws_bytes, void* ws,
    size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ clustering
 * DBSCAN (reference PointCloud.py:921-927: sklearn.cluster.DBSCAN(eps,
 * min_samples).fit(get_points()).labels_), additive to ABI 7.  The labels are
 * sklearn's, a deterministic function of the input:
 *   1. neighbourhood: j is a neighbour of i when d^2(i,j) <= eps*eps —
 *      inclusive, unlike the strict < of the Open3D radius searches above —
 *      and i is its own neighbour; d^2 = ((dx dx) + dy dy) + dz dz in float64
 *      on the float64 coordinates (float32 points upcast exactly);
 *   2. core: |N(i)| >= min_samples;
 *   3. clusters: the connected components of the core points under the
 *      neighbour relation, numbered 0, 1, ... in ascending order of each
 *      component's smallest core index;
 *   4. border: a non-core point with at least one core neighbour takes the
 *      smallest label among its core neighbours;
 *   5. noise: every other point is -1.
 * labels_dev (n int32) and core_dev (n bytes, 1 = core; nullable) are in the
 * original point order; *n_clusters_host receives the cluster count.  The
 * coordinates must be finite.  The result does not depend on launch order (no
 * float atomics).  o3dx_dbscan_f64 decides every pair from the caller's
 * float64 coordinates (the float64 boundary above).
 * Errors, checked before any device call: EINVAL for n <= 0, n >= 2^31,
 * eps <= 0 or not finite, min_samples < 1, a null xyz / labels /
 * n_clusters_host; ENOMEM for a workspace below o3dx_dbscan*_workspace_bytes(n)
 * (0 for an n outside the range).  EIO if the union-find's iteration bound is
 * exceeded (never, unless memory is corrupted).  Synchronises the stream. */
size_t o3dx_dbscan_workspace_bytes(int64_t n);
int o3dx_dbscan(const float* xyz_dev, int64_t n, double eps, int min_samples, int32_t* labels_dev,
                uint8_t* core_dev, int64_t* n_clusters_host, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_dbscan_f64_workspace_bytes(int64_t n);
int o3dx_dbscan_f64(const double* xyz_dev, int64_t n, double eps, int min_samples, int32_t* labels_dev,
                    uint8_t* core_dev, int64_t* n_clusters_host, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------- floor-map segmentation
 * Rasterisation, image labelling and grouping behind the reference's
 * to_2D_Img (PointCloud.py:785-823), simple_seg_connected_components and
 * simple_seg_connected_components_by_img (PointCloud.py:888-916) and
 * Processors.SimpleSegConnectedComponents (processors.py:772-799); additive to
 * ABI 7.
 *
 * Rasterisation.  bounds_host = {minx, miny, maxx, maxy} of the cloud's x and
 * y (float64; float32 points upcast exactly).  With ir = 1 / resolution,
 * tx = ir * (-minx), ty = ir * (-miny), every operation rounded to float64 on
 * its own (no fused multiply-add):
 *     ix = (int) rint(x * ir + tx),   iy = (int) rint(y * ir + ty)
 * (rint: round half to even, numpy's round).  The image is h rows of w pixels,
 * w = rint(maxx * ir + tx), h = rint(maxy * ir + ty): the largest ix / iy of
 * the cloud, both maps being monotone.  ix is then clamped to [0, w - 1] and
 * iy to [0, h - 1] — the last column and row fold into the one before, as in
 * the reference.  o3dx_raster2d_size (host only) returns {w, h} in wh_host;
 * either may be 0 (every point in one pixel column or row: the reference's
 * indexing raises there, and o3dx_raster2d returns EINVAL).  o3dx_raster2d /
 * o3dx_raster2d_f64 write pix_dev (n x 2 int32, {ix, iy}), clear img_dev
 * (h x w uint8, img_cap >= w * h pixels) and store 255 on every hit pixel;
 * winner_dev (h x w int32, nullable) receives the highest point index on each
 * pixel, -1 on an empty one (numpy's fancy assignment lets the last write
 * win: the colour image is built from it on the host).  Enqueue only; the
 * coordinates must be finite (a NaN lands on pixel 0, never outside).
 * Errors, before any device call: EINVAL for a resolution <= 0 or not finite,
 * null or non-finite bounds, max < min, n outside [1, 2^31), a null pointer, an
 * empty image; ENOTSUP for w * h >= 2^31; ENOMEM for img_cap < w * h.
 *
 * Connected components.  Foreground: a non-zero pixel; connectivity 8; label
 * 0 is the background; the components are numbered 1, 2, ... in ascending
 * row-major position of their first pixel (the smallest y * w + x; this is
 * also scipy.ndimage.label's numbering.  cv2 numbers by first 2 x 2 block
 * instead; the numbering is observable only through ties of equal area).
 * labels_dev: h x w int32.  areas_dev: int64, o3dx_ccl2d_max_labels(w, h) + 1
 * = ceil(w / 2) * ceil(h / 2) + 1 entries, of which [0, *n_labels_host] are
 * written: areas[l] = pixel count of label l, areas[0] = the zero pixels.
 * Tile-local labelling in LDS, a global union-find on the tile seams only;
 * integer atomics, the result does not depend on launch order.  Synchronises.
 * Errors, before any device call: EINVAL for w < 1, h < 1 or a null pointer;
 * ENOTSUP for w * h >= 2^31; ENOMEM for a workspace below
 * o3dx_ccl2d_workspace_bytes(w, h) (0 outside the range).
 *
 * Grouping.  point_label_dev[i] = labels_dev[iy_i * w + ix_i] for pix_dev
 * (n x 2 int32); order_dev (n int32): the point indices grouped by label,
 * ascending inside each label (a stable radix sort of ceil(log2(n_labels + 1))
 * bits); counts_dev (int64, n_labels + 1): points per label.  Synchronises.
 * EINVAL (after the device pass) if a pixel lies outside the image or a label
 * outside [0, n_labels]; before any device call EINVAL for n outside
 * [1, 2^31), a bad image size or a null pointer, ENOMEM for a workspace below
 * o3dx_label_group_workspace_bytes(n, n_labels). */
int o3dx_raster2d_size(double resolution, const double* bounds_host, int64_t* wh_host);
int o3dx_raster2d(const float* xyz_dev, int64_t n, double resolution, const double* bounds_host, int32_t* pix_dev,
                  uint8_t* img_dev, int32_t* winner_dev, int64_t img_cap, void* stream);
int o3dx_raster2d_f64(const double* xyz_dev, int64_t n, double resolution, const double* bounds_host,
                      int32_t* pix_dev, uint8_t* img_dev, int32_t* winner_dev, int64_t img_cap, void* stream);
size_t o3dx_ccl2d_workspace_bytes(int64_t w, int64_t h);
int64_t o3dx_ccl2d_max_labels(int64_t w, int64_t h);
int o3dx_ccl2d(const uint8_t* img_dev, int64_t w, int64_t h, int32_t* labels_dev, int64_t* areas_dev,
               int64_t* n_labels_host, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_label_group_workspace_bytes(int64_t n, int64_t n_labels);
int o3dx_label_group(const int32_t* pix_dev, int64_t n, const int32_t* labels_dev, int64_t w, int64_t h,
                     int64_t n_labels, int32_t* point_label_dev, int32_t* order_dev, int64_t* counts_dev, void* ws,
                     size_t ws_bytes, void* stream);

/* --------------------------- spanning trees and consistent normal orientation
 * Open3D 0.19 OrientNormalsConsistentTangentPlane(k) (reference
 * PointCloud.py:69-70, estimate_normals(method="poisson")); additive to ABI 7.
 * Every edge comparison uses one strict total order on undirected edges,
 * (w, min(i,j), max(i,j)), so both trees are unique — duplicate points and
 * lattices included — and the result does not depend on launch order.
 *
 * o3dx_emst: the Euclidean minimum spanning tree of the n points, the MST of
 * the complete graph under w = d^2(i,j) = ((dx dx) + dy dy) + dz dz in float64
 * on the float32 coordinates upcast exactly.  Open3D finds the same tree
 * inside the Delaunay edges; here it is Boruvka rounds over the search grid,
 * so fewer than 4 points or coplanar points simply work.  edges_out_dev:
 * (n - 1, 2) int32 rows {lo, hi}, lo < hi, sorted by (lo, hi).  knn_idx_dev /
 * k: the points' neighbour lists when the caller has them (nullable, k >= 0;
 * a hint only, unused at present).
 *
 * o3dx_orient_normals_tangent_plane, given each point's neighbour list
 * knn_idx_dev ((n, k) int32, o3dx_knn_search's rows on the cloud itself with
 * knn = min(k, n); entries < 0 and the point itself are skipped):
 *   1. the Riemannian graph = the arcs {i, knn[i][*]} united with the EMST;
 *   2. its MST under w = 1.0 - |dot|, dot = ((nx nx') + ny ny') + nz nz' in
 *      float64 on the float32 normals, no fused multiply-add;
 *   3. the root is the lowest index among the points of maximal z, flipped
 *      iff its nz < 0; along the tree a child is flipped iff
 *      dot(parent as oriented, child) < 0 (dot == 0 never flips), i.e.
 *      flip[i] = flip[root] ^ (the number of tree edges with dot < 0 on the
 *      path root -> i, mod 2);
 *   4. a flipped normal has its three sign bits toggled in normals_inout_dev;
 *      magnitudes stay bit-identical.
 * tree_out_dev (nullable): the (n - 1, 2) tree edges as o3dx_emst writes them;
 * flipped_out_dev (nullable): n bytes, 1 = flipped.  Open3D 0.18+'s lambda /
 * cos_alpha_tol arguments are not offered (their defaults are inert).
 * Coordinates and normals must be finite.
 * Errors, before any device call: EINVAL for n outside [1, 2^31), k < 0
 * (o3dx_emst) or k < 1, a null xyz / edges (n > 1) / knn_idx / normals; ENOMEM
 * for a workspace below o3dx_*_workspace_bytes (0 for arguments outside the
 * range).  EIO for a HIP error, a raised iteration bound, or a tree that does
 * not reach n - 1 edges (non-finite input).  At most ceil(log2 n) rounds per
 * tree, one small host read per round.  Synchronises the stream. */
size_t o3dx_emst_workspace_bytes(int64_t n);
int o3dx_emst(const float* xyz_dev, int64_t n, const int32_t* knn_idx_dev, int k, int32_t* edges_out_dev, void* ws,
              size_t ws_bytes, void* stream);
size_t o3dx_orient_normals_workspace_bytes(int64_t n, int k);
int o3dx_orient_normals_tangent_plane(const float* xyz_dev, int64_t n, const int32_t* knn_idx_dev, int k,
                                      float* normals_inout_dev, int32_t* tree_out_dev, uint8_t* flipped_out_dev,
                                      void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- LAS IO
 * LAS 1.0-1.4 point records, uncompressed, on the device; additive to ABI 7.
 * Replaces the laspy record handling behind the reference's LAS methods
 * (reference PointCloud.py:496-567: read_las / read_las_gen 523-547,
 * get_lasdata / append_save_las / save_las 499-521, 549-565).  The host parses
 * and writes the public header (las_io.py); records are `stride` bytes each
 * (the header's record length: at least the format's minimum, any extra bytes
 * are skipped on reading and zero on writing; no alignment needed).  In every
 * format X, Y, Z are int32 at 0, 4, 8 and the intensity a u16 at 12; the
 * classification byte is at 15 (formats 0-5) or 16 (6-10); red, green, blue
 * are u16 at 20 (format 2), 28 (3, 5) or 30 (7, 8, 10).  scale_host /
 * offset_host: 3 doubles each, finite, scale non-zero.
 *
 * o3dx_las_unpack (formats 0..10): per record and axis
 *   x = (double)X * scale + offset      (one multiply, then one add; no fma)
 * into xyz64_out_dev ((n,3) float64) and, rounded once, xyz32_out_dev ((n,3)
 * float32); intensity_out_dev (n) the raw u16; cls_out_dev (n) the whole
 * classification byte (laspy's raw_classification for formats 0-5; byte 16 for
 * 6+, where laspy has no such field); rgb_out_dev ((n,3) float32) = u16 / 65536
 * (exact).  Every output is nullable.  flags_dev (nullable, one u32) is
 * cleared, then gets O3DX_LAS_FLAG_NOT_F32 when some x is not a float32 value
 * (NaN does not count).  EINVAL for a format outside 0..10, a stride below
 * the format's minimum or above 65535, and rgb_out_dev on a format without
 * colour.  n = 0 is allowed.  Enqueues only.
 *
 * o3dx_las_pack (formats 0..3, 6..8): rec_out_dev (n * stride bytes) is
 * zero-filled and receives, per record and axis,
 *   X = rint((x - offset) / scale)      (float64, ties to even: np.round)
 * from xyz_dev ((n,3) float64 when xyz_f64, else float32 upcast exactly);
 * rgb_dev ((n,3) float32, nullable) as (uint8)(c * 255.0) — the product in
 * float64, truncated — stored in the u16 colour fields, as the reference's
 * get_lasdata does (so a colour read back through / 65536 is dimmed 256-fold);
 * intensity_dev (n u16, nullable) and cls_dev (n u8, nullable) as they are.
 * stats_dev, 8 int64: {min X, min Y, min Z, max X, max Y, max Z} over the
 * values that fit int32 (INT32_MAX / INT32_MIN when there is none), the count
 * of values outside int32 and the count of non-finite values (both are stored
 * as 0 in the record).  EINVAL as above, and for rgb_dev on a format without
 * colour.  n = 0 is allowed (the statistics are still initialised).  Enqueues
 * only: the caller waits when it reads the statistics. */
#define O3DX_LAS_FLAG_NOT_F32 1u
int o3dx_las_unpack(const uint8_t* rec_dev, int64_t n, int64_t stride, int point_format, const double* scale_host,
                    const double* offset_host, double* xyz64_out_dev, float* xyz32_out_dev,
                    uint16_t* intensity_out_dev, uint8_t* cls_out_dev, float* rgb_out_dev, uint32_t* flags_dev,
                    void* stream);
int o3dx_las_pack(const void* xyz_dev, int xyz_f64, int64_t n, int64_t stride, int point_format,
                  const double* scale_host, const double* offset_host, const float* rgb_dev,
                  const uint16_t* intensity_dev, const uint8_t* cls_dev, uint8_t* rec_out_dev, int64_t* stats_dev,
                  void* stream);

/* ---------------------------------------------------------------- E57 IO
 * E57 (ASTM E2807) files on the device; additive to ABI 7.  Replaces the
 * pye57 / libE57 byte work behind the reference's E57 methods (reference
 * PointCloud.py:569-703, E57File.py).  The host (e57_io.py) parses and writes
 * the 48-byte file header, the XML, the section headers and the packet
 * headers.  The file's bytes are in device memory once, paged as on disk: a
 * page is 1024 bytes, 1020 of payload and a big-endian CRC32C (Castagnoli:
 * reflected 0x82F63B78, init and final xor 0xFFFFFFFF) of them; logical
 * offset l is physical offset l + 4 * (l / 1020).
 *
 * o3dx_e57_crc_pages: checks the n_pages pages at file_dev (16-byte aligned);
 * out2_dev = {bad pages, first bad page or INT64_MAX}.
 *
 * o3dx_e57_unpack decodes records [r0, r0 + n) of one scan.  desc_host, 6
 * int64 per field: {role O3DX_E57_ROLE_*, kind O3DX_E57_KIND_*, bits, minimum,
 * first segment row, segment rows}; affine_host, 2 doubles per field: {scale,
 * offset}.  seg_dev: rows {stream byte offset, logical file offset, length} of
 * the field's bytestream, ascending and gap-free in the stream (the pieces of
 * it in the data packets), lengths > 0.  Record r of a field of b bits is the
 * b bits from stream bit r * b, LSB first; bytes that are not contiguous in
 * the file are fetched one by one, so a value may straddle a page trailer and
 * a segment end.  Rules:
 *   Float single widens to float64 exactly; Float double as it is;
 *   Integer        v = minimum + raw                     (int64, wrapping)
 *   ScaledInteger  x = (double)v * scale + offset        (one multiply, then
 *                                                         one add; no fma)
 *   pose_host (nullable; 12 doubles, R row-major then t):
 *     x' = ((R00 * x + R01 * y) + R02 * z) + t0          (in that order)
 * Outputs, each nullable: xyz64 (n,3) float64, xyz32 (n,3) float32 (rounded
 * once), rgb (n,3) uint8, intensity (n) float32 (an Integer field converts
 * with one rounding), row / col (n) uint16, invalid (n) int8 — the integer
 * columns take Integer fields only and keep the low bits.  A field whose
 * output is null is not decoded.  flags_dev (nullable, one u32) is cleared,
 * then gets O3DX_E57_FLAG_NOT_F32 when some output coordinate is not a float32
 * value (NaN does not count) and O3DX_E57_FLAG_RANGE when a record's bytes lie
 * outside its segments or the file (they read as 0; nothing outside file_dev
 * is touched).  EINVAL for a role twice, a kind / bits mismatch, segment rows
 * outside the table and an output without its field(s).  Enqueues only.
 *
 * o3dx_e57_pack writes the data packets of one scan, headers included, into
 * out_dev (4-byte aligned; (packets - 1) * full_bytes + last_bytes bytes,
 * every byte written).  Packets hold records_per_packet records (a multiple
 * of 8, so every stream is whole bytes), the last one the rest; head_full_host
 * / head_last_host are their 6 + 2 * n_fields header bytes.  desc_host, 6
 * int64 per field: {source O3DX_E57_SRC_*, bits, minimum, stream offset in a
 * full packet, in the last packet, stream bytes in the last packet}; src_host:
 * one device pointer per field; stride_host: {element stride, first element}
 * per field.  Sources: F32 / F64 the value's bits (32 / 64); COLOUR a float32
 * colour as (uint8)(c * 255.0), the product in float64, truncated (8 bits);
 * I64 an int64 as value - minimum in `bits` bits (0..64).  Bit-packed streams
 * are gathered: one lane per output word collects the records overlapping it.
 *
 * o3dx_e57_seal lays logical_bytes (a multiple of 4) into n_pages pages at
 * paged_out_dev, zero-pads the last and writes each page's CRC trailer. */
#define O3DX_E57_ROLE_X 0
#define O3DX_E57_ROLE_Y 1
#define O3DX_E57_ROLE_Z 2
#define O3DX_E57_ROLE_INTENSITY 3
#define O3DX_E57_ROLE_RED 4
#define O3DX_E57_ROLE_GREEN 5
#define O3DX_E57_ROLE_BLUE 6
#define O3DX_E57_ROLE_ROW 7
#define O3DX_E57_ROLE_COLUMN 8
#define O3DX_E57_ROLE_INVALID 9
#define O3DX_E57_KIND_F32 0
#define O3DX_E57_KIND_F64 1
#define O3DX_E57_KIND_INT 2
#define O3DX_E57_KIND_SCALED 3
#define O3DX_E57_SRC_F32 0
#define O3DX_E57_SRC_F64 1
#define O3DX_E57_SRC_COLOUR 2
#define O3DX_E57_SRC_I64 3
#define O3DX_E57_FLAG_NOT_F32 1u
#define O3DX_E57_FLAG_RANGE 2u
int o3dx_e57_crc_pages(const uint8_t* file_dev, int64_t n_pages, int64_t* out2_dev, void* stream);
int o3dx_e57_unpack(const uint8_t* file_dev, int64_t file_bytes, int n_fields, const int64_t* desc_host,
                    const double* affine_host, const int64_t* seg_dev, int64_t seg_rows, int64_t r0, int64_t n,
                    const double* pose_host, double* xyz64_out_dev, float* xyz32_out_dev, uint8_t* rgb_out_dev,
                    float* intensity_out_dev, uint16_t* row_out_dev, uint16_t* col_out_dev, int8_t* invalid_out_dev,
                    uint32_t* flags_dev, void* stream);
int o3dx_e57_pack(int n_fields, const int64_t* desc_host, const void* const* src_host, const int64_t* stride_host,
                  int64_t n, int64_t records_per_packet, int64_t full_bytes, int64_t last_bytes,
                  const uint8_t* head_full_host, const uint8_t* head_last_host, uint8_t* out_dev, void* stream);
int o3dx_e57_seal(const uint8_t* logical_dev, int64_t logical_bytes, uint8_t* paged_out_dev, int64_t n_pages,
                  void* stream);

/* ------------------------------------- global registration (additive to ABI 7)
 * Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching
 * / _on_correspondence.  The semantics are Open3D's as restated in DESIGN.md
 * §4.11 (tests/globalreg_oracle.py is the executable form the tests pin).
 *
 * o3dx_fpfh: the (n,33) float32 FPFH of points with normals.  The neighbour
 *   lists are o3dx_knn_search(xyz, xyz, mode, knn, radius) — sorted by (d^2,
 *   index), the point itself included — taken once; mode KNN or HYBRID, knn
 *   <= O3DX_MAX_KNN (RADIUS: O3DX_ENOTSUP, unbounded lists).  All arithmetic
 *   float64 on the float32 inputs, rounded once to float32.  Pass 1 writes one
 *   36-byte SPFH row per point: the 33 integer bin counts (each <= 63), byte
 *   33 the list length m, bytes 34..35 zero; SPFH bin b = count_b * 100 / (m -
 *   1).  Pass 2 gathers the neighbours' rows.  spfh_out_dev (nullable, n x 36
 *   bytes) receives the rows.  Integer and fixed-order accumulation only: two
 *   runs give the same bits.
 * o3dx_feature_match: for each of ns source rows (33 float32) the target row
 *   (of nt >= 1) with the smallest squared distance, (a - b)^2 summed over the
 *   33 components in float32, component order; the lowest target index wins a
 *   tie.  idx_out_dev (ns) int32, d2_out_dev (nullable, ns) float32.
 * o3dx_umeyama_from_samples: host only.  coords_host (H x ransac_n x 2 x 3
 *   float64: the sampled source point, then its target point) -> T_host (H x
 *   16): TransformationEstimationPointToPoint(false) of each sample through
 *   o3dx_icp_solve_point_to_point (the identity for a rank-deficient sample).
 * o3dx_corr_check: host only.  pass_host[h] = 1 when sample h passes
 *   CorrespondenceCheckerBasedOnEdgeLength(edge_similarity) (skipped when
 *   edge_similarity < 0: fails if for any two sampled pairs |pi - pj| < |qi -
 *   qj| s or |qi - qj| < |pi - pj| s) and CorrespondenceCheckerBasedOnDistance
 *   (distance_threshold) (skipped when < 0: fails if any |T p - q| > t).
 * o3dx_corr_count: counts_host[h] = the exact number of correspondences
 *   (corr_dev: C x 2 int32, source and target index) with |T_h p - q| <
 *   max_distance.  float32 distance with a guard band around the threshold,
 *   inside which the decision is made again in float64 in the pinned order:
 *   T p = ((T0 x + T1 y) + T2 z) + T3 per row, d = sqrt((dx^2 + dy^2) + dz^2),
 *   strict <.  Integer ballots.
 * o3dx_corr_error2: sums_host[h] = sum of d * d over those inliers, float64 in
 *   a fixed order (counts_host nullable: the counts again). */
size_t o3dx_fpfh_workspace_bytes(int64_t n, int knn);
int o3dx_fpfh(const float* xyz_dev, const float* normals_dev, int64_t n, int mode, int knn, double radius,
              float* out_dev, uint8_t* spfh_out_dev, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_feature_match_workspace_bytes(int64_t ns, int64_t nt);
int o3dx_feature_match(const float* src_feat_dev, int64_t ns, const float* tgt_feat_dev, int64_t nt,
                       int32_t* idx_out_dev, float* d2_out_dev, void* ws, size_t ws_bytes, void* stream);
int o3dx_umeyama_from_samples(const double* coords_host, int num_hypotheses, int ransac_n, double* T_host);
int o3dx_corr_check(const double* coords_host, int num_hypotheses, int ransac_n, const double* T_host,
                    double edge_similarity, double distance_threshold, uint8_t* pass_host);
size_t o3dx_corr_count_workspace_bytes(int64_t c, int num_hypotheses);
int o3dx_corr_count(const float* src_dev, const float* tgt_dev, const int32_t* corr_dev, int64_t c,
                    const double* T_host, int num_hypotheses, double max_distance, int64_t* counts_host,
                    void* ws, size_t ws_bytes, void* stream);
int o3dx_corr_error2(const float* src_dev, const float* tgt_dev, const int32_t* corr_dev, int64_t c,
                     const double* T_host, int num_hypotheses, double max_distance, double* sums_host,
                     int64_t* counts_host, void* ws, size_t ws_bytes, void* stream);

/* ---- uncapped radius sweeps: neighbour count, ISS keypoints (additive to ABI 7)
 * One neighbourhood rule: j is in N_r(i) when d^2(i,j) < r * r (strict; i
 * itself is in), d^2 in float64 as ((dx dx) + dy dy) + dz dz on the float64
 * values of the coordinates (the rule of the radius normals).  The *_f64
 * entries decide every pair, and take every moment, from the caller's float64
 * coordinates.  radius finite and > 0, 1 <= n < 2^31, else EINVAL; ENOMEM for a
 * workspace below the entry's own *_workspace_bytes(n).  Outputs are
 * bit-identical run to run (no float atomics).
 *
 * o3dx_radius_count: count_dev[i] = min(|N_r(i)|, cap) (cap <= 0: no cap; the
 *   sweep of a point stops at cap).  Replaces the per-point SearchRadius of
 *   Open3D's PointCloud::RemoveRadiusOutliers (keep when the count > nb_points).
 * o3dx_iss_saliency: count_dev[i] = |N_r(i)| and s_dev[i], the ISS saliency of
 *   o3d.geometry.keypoint.compute_iss_keypoints (ComputeKeypointsISS' first
 *   loop): 0 when the count < min_neighbors or when every |entry| of the
 *   neighbours' covariance C (sum p p^T / k - mu mu^T, float64) is <= 1e-12;
 *   else with C's eigenvalues e1 >= e2 >= e3 (Eberly's non-iterative solve),
 *   s = e3 when e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (NaN ratios compare
 *   false), else 0.  s is a function of the neighbour SET alone: the moments
 *   are taken about the set's first member in cell-sorted order and added in
 *   ascending cell-sorted position per query, so two points with the same
 *   neighbours get the same bits (Open3D adds them in kd-tree result order).
 * o3dx_iss_nms: ComputeKeypointsISS' second loop.  i is a keypoint when
 *   s[i] > 0, |N_r(i)| >= min_neighbors and no j in N_r(i) has s[i] < s[j]
 *   (strict: exact ties both survive).  idx_out_dev (capacity n) receives the
 *   keypoints in ascending index order (Open3D's order is arbitrary),
 *   *count_host their number.
 * o3dx_nn_distance_sum: *sum_host = the sum of sqrt(d2_dev[i * k + col]) over
 *   the rows with cnt_dev[i] > col, float64 in a fixed order (ComputeModel-
 *   Resolution's sum over a 2-NN search: k = 2, col = 1).  ws: >= 256 bytes. */
size_t o3dx_radius_count_workspace_bytes(int64_t n);
int o3dx_radius_count(const float* xyz_dev, int64_t n, double radius, int cap, int32_t* count_dev, void* ws,
                      size_t ws_bytes, void* stream);
size_t o3dx_radius_count_f64_workspace_bytes(int64_t n);
int o3dx_radius_count_f64(const double* xyz_dev, int64_t n, double radius, int cap, int32_t* count_dev, void* ws,
                          size_t ws_bytes, void* stream);
size_t o3dx_iss_saliency_workspace_bytes(int64_t n);
int o3dx_iss_saliency(const float* xyz_dev, int64_t n, double radius, double gamma_21, double gamma_32,
                      int min_neighbors, double* s_dev, int32_t* count_dev, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_iss_saliency_f64_workspace_bytes(int64_t n);
int o3dx_iss_saliency_f64(const double* xyz_dev, int64_t n, double radius, double gamma_21, double gamma_32,
                          int min_neighbors, double* s_dev, int32_t* count_dev, void* ws, size_t ws_bytes,
                          void* stream);
size_t o3dx_iss_nms_workspace_bytes(int64_t n);
int o3dx_iss_nms(const float* xyz_dev, int64_t n, const double* s_dev, double radius, int min_neighbors,
                 int32_t* idx_out_dev, int64_t* count_host, void* ws, size_t ws_bytes, void* stream);
size_t o3dx_iss_nms_f64_workspace_bytes(int64_t n);
int o3dx_iss_nms_f64(const double* xyz_dev, int64_t n, const double* s_dev, double radius, int min_neighbors,
                     int32_t* idx_out_dev, int64_t* count_host, void* ws, size_t ws_bytes, void* stream);
int o3dx_nn_distance_sum(const double* d2_dev, const int32_t* cnt_dev, int64_t n, int k, int col, double* sum_host,
                         void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* O3DX_H */
