/*
 * vcp.h -- C-ABI of libvcp.so: MI355X (gfx950) DBSCAN + centroid + ICP hot path of
 * ZhiHuangHn/vtkCloudPoint.  Plain pointers and sizes only; no C++/torch types.
 *
 * Each entry point replaces one piece of the reference's C# class surface; the citation
 * (file:line under /root/reference/vtkPointCloud/, BC = BaseClass) names what it stands in
 * for.  The C# side binds these with [DllImport("vcp")] -- see INTEGRATION.md.
 *
 * Conventions
 *  - every call is blocking and re-entrant per context (one vcp_ctx per caller thread, the
 *    way FrmMain.cs:1358 runs one DBImproved per pool thread); the library keeps no pointer
 *    after a call returns;
 *  - return value: 0 = VCP_OK, < 0 = error (vcp_last_error(ctx) gives the text);
 *  - "host" entry points take caller-owned host buffers and do H2D/D2H themselves;
 *    "_dev" entry points take device pointers (inputs already resident in HBM) and run on
 *    the context's stream;
 *  - there is NO CPU fallback: without a HIP device every compute call fails with
 *    VCP_ERR_NO_DEVICE.
 */
#ifndef VCP_H
#define VCP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCP_VERSION_MAJOR 0
#define VCP_VERSION_MINOR 1

typedef struct vcp_ctx vcp_ctx;

/* distance forms: BC/DBImproved.cs:21 (live, |dx|+|dy| on motor_x/motor_y), :24 and :20
 * (commented-out Euclidean 2-D / 3-D), BC/DB.cs:21 (dead v1.0 class, signed dx+dy). */
enum vcp_metric { VCP_L1_2D = 0, VCP_L2_2D = 1, VCP_L2_3D = 2, VCP_SIGNED_SUM_2D = 3 };

/* ICP stop rules: BC/ICP.cs:180 (|SSE - previous SSE| < e) or RMSE = sqrt(SSE/Nd) < e. */
enum vcp_icp_stop { VCP_STOP_SSE_DELTA = 0, VCP_STOP_RMSE = 1 };

enum vcp_status {
  VCP_OK = 0,
  VCP_ERR_ARG = -1,          /* invalid argument                                           */
  VCP_ERR_EMPTY = -2,        /* the C# would throw on an empty collection                  */
  VCP_ERR_DEGENERATE = -3,   /* zero-extent first block: rows/cols undefined               */
  VCP_ERR_INDEX = -4,        /* the C# would throw IndexOutOfRange / ArgumentOutOfRange    */
  VCP_ERR_TOO_LARGE = -5,    /* n or grid beyond 32-bit indexing                           */
  VCP_ERR_NO_DEVICE = -6,    /* no HIP device / device id out of range                     */
  VCP_ERR_HIP = -7,          /* HIP runtime error                                          */
  VCP_ERR_UNSUPPORTED = -8,  /* valid request this build does not run on the GPU           */
  VCP_ERR_NOMEM = -9
};

/* -- context ------------------------------------------------------------------------------ */
/* device_id: HIP ordinal (one context drives one GPU; several GPUs: vcp_create_multi below, or one process per GPU). */
int vcp_create(int device_id, vcp_ctx** out);
void vcp_destroy(vcp_ctx* ctx);
const char* vcp_last_error(const vcp_ctx* ctx); /* ctx may be NULL: last create error      */
int vcp_version(void);                           /* major*1000 + minor                      */
/* Run on a caller-provided hipStream_t: from this call on every kernel, copy, memset and event of the context goes to
 * hip_stream, the host-buffer entry points and vcp_h2d / vcp_d2h included.
 *  - the inputs of a call must be ordered on that stream: work the caller queued on it before the call (a copy that
 *    fills an input buffer, a kernel that produces it) is seen by the call; work on any other stream is not waited for;
 *  - a call returns when its work on the stream is done, so everything queued on the stream before it is done too;
 *  - the stream must outlive its use by the context: select another one (or NULL) or destroy the context first;
 *  - NULL selects the context's own stream (created non-blocking by vcp_create), so the legacy null stream cannot be
 *    selected.
 * The workspace may grow during a call on any stream.  tests/test_stream_gpu.py holds every _dev entry point to this. */
int vcp_set_stream(vcp_ctx* ctx, void* hip_stream);
/* Pinned-free device allocation helpers for hosts without a HIP binding of their own (the C# and C++ way of keeping a
 * cloud resident): alloc, h2d, the _dev call, d2h, free.  bytes == 0 allocates a valid pointer vcp_dev_free accepts;
 * the copies run on the context's stream and return when done (bytes == 0 copies nothing).  ctx == NULL, a NULL dptr /
 * device pointer, or a NULL host pointer with bytes > 0: VCP_ERR_ARG. */
int vcp_dev_alloc(vcp_ctx* ctx, uint64_t bytes, void** dptr);
int vcp_dev_free(vcp_ctx* ctx, void* dptr);
int vcp_h2d(vcp_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);
int vcp_d2h(vcp_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);

/* The context keeps its device workspace between calls (no hipMalloc on the steady-state path; ~100 bytes per
 * point of the largest call so far).  This frees it -- and the staged block / slab state -- without destroying the
 * context; the next call allocates again. */
int vcp_release_workspace(vcp_ctx* ctx);

/* Self-test of the library's device prefix scan (every pipeline stage places its output with it): exclusive sum
 * (op 0) or exclusive running maximum (op 1) of d_in [n] u32 into d_out [n] (d_out == d_in allowed), grand total to
 * *total.  Device pointers; returns when the result is in place. */
int vcp_selftest_scan_dev(vcp_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, int64_t n, int op, uint32_t* total);

/* Test hook: overwrite everything a call may not rely on.  armed != 0: waits for the context's stream, fills every
 * workspace buffer the context lists over its whole capacity, the pinned scratch and the staging area with the 32-bit
 * `word`, waits again, and reports the device buffers filled and their bytes -- device memory only, the two pinned areas
 * are not counted -- (either pointer may be NULL).  The context
 * stays armed: from then on every fresh allocation of the workspace and of the staging area is filled with the word
 * before its first use, so fresh memory never looks initialised.  armed == 0 disarms and fills nothing.
 * Left alone: the buffers that carry state across calls by design (the scan's descriptors, the output partition's window
 * cursors: the array k_poison_left_alone in csrc/vcp_ctx.hip gives the reasons) and the buffers a staged state owns.
 * For use between independent calls ONLY: never between the stages of the vcp_blocks_... or vcp_slab_... sequences, whose
 * later stages read what the earlier ones left in the workspace.  The steady-state path pays one never-taken branch
 * where a buffer grows. */
int vcp_selftest_poison(vcp_ctx* ctx, int armed, uint32_t word, uint64_t* filled_bytes, int32_t* filled_bufs);
/* Test hook: sets the generation number of the scan's descriptors (30 bits; VCP_ERR_ARG beyond), to reach its wrap
 * (memset, restart at 1) without 2^30 scans.  Only raise it: a generation the context has used may still stand in a
 * descriptor. */
int vcp_selftest_scan_generation(vcp_ctx* ctx, uint32_t gen);

/* Self-test of the Horn step of vcp_icp (BC/ICP.cs:53-124, intended arithmetic), run on the HOST from the same source
 * the device executes per round: sums[16] as vcp_icp_sums returns them, nd data points.  use_v != 0: V [16] is the
 * eigenvector basis of a previous round (warm start; a basis that is not orthonormal to 1e-9 -- NaN included -- is
 * replaced by the identity) and receives the basis found.  Returns 1 (solved), 0 (failed) or VCP_ERR_ARG (NULL sums,
 * R1 or T1, nd <= 0, use_v without V).  sums[15] is not read.
 * 1 means: R1 is orthonormal with det +1 to 32 u (u = 2^-53), maximises sum_ab R[a][b] m[b][a] to 64 u big, and lies
 * within 150 u (cond + 1) of the exact solution of the same sums, T1 within 150 u (cond + 1)(|muP|max + 1) + 4 u |T1|,
 * where m = S/N - muP muY^T, big = max(|sums[6..14]|/nd, |muP_a muY_b|) and cond = big over the gap between the two
 * largest eigenvalues of Horn's 4x4 matrix (a tie, e.g. a collinear cloud: any of the equally good rotations).  That
 * holds for every finite input whose means, products muP_a muY_b and sums/nd stay normal binary64 numbers: the step is
 * exactly invariant under a power-of-two scaling of the coordinates (R1 bit-identical, T1 scaled).  All-zero sums are
 * coincident points: R1 = I, T1 = 0.  Outside that range -- NaN or an infinity in any of sums[0..14], or sums so large
 * that Horn's matrix overflows -- the answer is 0 and R1 and T1 are not written.  cond grows with the square of the
 * clouds' distance from the origin: see DESIGN.md, "Accuracy of the Horn step".
 * Needs no device and no context. */
int vcp_selftest_horn(const double sums[16], int64_t nd, double V[16], int use_v, double R1[9], double T1[3]);

/* -- per-phase device timing (hipEvents on the launch stream) ----------------------------- */
/* When enabled, every compute call records hipEvents around each kernel phase on the stream
 * it launches on.  vcp_timing_get returns the phases of the LAST call. */
int vcp_timing_enable(vcp_ctx* ctx, int on);
int vcp_timing_count(vcp_ctx* ctx);
int vcp_timing_get(vcp_ctx* ctx, int i, const char** name, float* ms);

/* -- DBSCAN -------------------------------------------------------------------------------
 * Replaces DBImproved.dbscan(List<Point3D> lst, double e, int minPts), BC/DBImproved.cs:91-114
 * (with isKeyPoint :33-54 and expandCluster :56-90), call sites FrmMain.cs:1507-1516,
 * :2785-2786, BC/Tools.cs:591-592.  Exact semantics:
 *   core[i]      <=> #{j : d(i,j) <= eps} >= min_pts (the count includes i)
 *   expanding[i] <=> core[i] and not in_classed[i]
 *   clusters      = connected components of the expanding points under d <= eps, numbered
 *                   cf_in+1, cf_in+2, ... by increasing smallest member index
 *   any other point within eps of an expanding point takes the LARGEST such cluster id
 *                   (BC/DBImproved.cs:87 relabels unconditionally); otherwise it is untouched
 * coords     [n*dim] doubles, point-major (x,y[,z]); dim 2 or 3; the 2-D metrics read x,y
 * cf_in      DBImproved.cf before the call (FrmMain.cs:1509 presets it)
 * in_mask    ifShown filter of BC/DB.cs:40,63,98 -- only with VCP_SIGNED_SUM_2D, the dead v1.0 class DB
 *            (BC/DB.cs:14-115, FrmMain.cs:38): signed distance dx + dy on (x, y), clusters numbered from cf_in + 1,
 *            dist_evals = DB.iritatorNum, DB.pointsAmount = the number of shown points.  Sorts and scans where the
 *            class's floating-point relation is provably the 1-D relation on x + y (eps >= 0, finite coordinates, a
 *            common binary grid or no pair within rounding of the threshold: csrc/dbdead.hip); every other input --
 *            eps < 0 or NaN, non-finite coordinates included -- pair by pair, O(n^2), up to 2^21 points
 *            (csrc/dbpairs.hip; VCP_ERR_UNSUPPORTED beyond)
 * in_classed NULL = nobody classed and labels start at 0 (what every caller sets up,
 *            FrmMain.cs:1219-1223, :1512-1515); else Point3D.isClassed on entry and `labels`
 *            is read as Point3D.clusterId on entry
 * labels     [n] out (in/out with in_classed): Point3D.clusterId
 * is_core    [n] out, may be NULL: isKeyPoint flags SET by this call (core and queried)
 * is_classed [n] out, may be NULL: Point3D.isClassed after the call
 * cf_out     DBImproved.cf / clusterAmount after the call
 * dist_evals DBImproved.iritatorNum increment as a 64-bit count (BC/DBImproved.cs:12,19):
 *            what the O(n^2) C# would have evaluated, not what the GPU evaluates
 */
int vcp_dbscan(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, double eps,
               int min_pts, int32_t cf_in, const uint8_t* in_mask, const uint8_t* in_classed,
               int32_t* labels, uint8_t* is_core, uint8_t* is_classed, int32_t* cf_out,
               int64_t* dist_evals);
/* Same with device pointers; cf_out / dist_evals stay host pointers (16 bytes read back). */
int vcp_dbscan_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, double eps,
                   int min_pts, int32_t cf_in, const uint8_t* d_in_classed, int32_t* d_labels,
                   uint8_t* d_is_core, uint8_t* d_is_classed, int32_t* cf_out, int64_t* dist_evals);

/* -- block-partitioned DBSCAN ("v2.0 multithread") ----------------------------------------
 * Replaces MainForm.getClusterFromMotor (FrmMain.cs:1214-1291: sort, first-block size, (lo,hi]
 * rectangle blocks via Tools.getListByScale2 BC/Tools.cs:510-513), StartCode (:2782-2794: one
 * DBImproved per block) and CompleteWork3 (:1442-1520: renumber, demote clusters of
 * <= small_max points, one global DBImproved over all noise with cf preset).
 * motor [n*2]; labels [n] by original index (0 = noise or dropped); block_of [n] may be NULL
 * (-1 = in no block); merge_order [n] may be NULL: original indices in final clusForMerge
 * order, *m_out entries.  kept = clusters surviving the demotion, del_sum = demoted clusters,
 * cluster_amount = DBImproved.clusterAmount after the noise pass (FrmMain.cs:1521-1522).
 * Limits: rows * cols <= 2^26 - 4 blocks (VCP_ERR_TOO_LARGE beyond: the C#'s cells[,] would be a 4 GB array of list
 * references there); a first block of zero extent = VCP_ERR_DEGENERATE (the C# divides by it, :1256-1259). */
int vcp_dbscan_blocks(vcp_ctx* ctx, const double* motor, int64_t n, double eps, int min_pts,
                      int pts_in_cell, int small_max, int32_t* labels, int32_t* block_of,
                      int64_t* merge_order, int64_t* m_out, int32_t* rows, int32_t* cols,
                      int32_t* kept, int32_t* del_sum, int32_t* cluster_amount, int64_t* dist_evals);

/* The 3-D twin MainForm.getClusterFromList (FrmMain.cs:1136-1213 with Tools.getListByScale, BC/Tools.cs:507-509): the
 * same pipeline, but the PARTITION (bounds, sort key, first-block size, (lo,hi] rectangles) reads key_xy [n*2] = (X, Y)
 * while every DBImproved -- per block and the noise pass -- still clusters on motor [n*2] (StartCode :2785-2786).
 * key_xy == NULL is vcp_dbscan_blocks. */
int vcp_dbscan_blocks_keyed(vcp_ctx* ctx, const double* key_xy, const double* motor, int64_t n, double eps,
                            int min_pts, int pts_in_cell, int small_max, int32_t* labels, int32_t* block_of,
                            int64_t* merge_order, int64_t* m_out, int32_t* rows, int32_t* cols, int32_t* kept,
                            int32_t* del_sum, int32_t* cluster_amount, int64_t* dist_evals);

/* The same pipeline in three stages, for sharding the per-block step over several GPUs (one
 * process and one context per GPU, every rank holds the whole cloud; SURVEY.md 8e mode 1):
 *   begin    partition (deterministic, identical on every rank); *m = points that fell in a block
 *   share    contiguous block range of `rank`, balanced on point count, and the matching
 *            [pos_lo, pos_hi) slice of the block-major label array
 *   cluster  DBImproved per block for block_lo <= b < block_hi; writes the block-local cluster ids
 *            (cf starts at 0 in every block, FrmMain.cs:2785) into d_local[pos_lo..pos_hi)
 *   -- the caller all-gathers the slices of d_local (RCCL) and sums the per-rank evals --
 *   finish   CompleteWork3 on the full d_local [m]; d_* outputs are device pointers
 * The state lives in the context until the next begin.  The _dev forms of begin read d_motor (and d_key_xy) in
 * place: the caller keeps those arrays valid and unchanged until the finish stage has returned. */
int vcp_blocks_begin(vcp_ctx* ctx, const double* motor, int64_t n, double eps, int min_pts,
                     int pts_in_cell, int small_max, int32_t* rows, int32_t* cols, int64_t* nblocks,
                     int64_t* m);
int vcp_blocks_begin_dev(vcp_ctx* ctx, const double* d_motor, int64_t n, double eps, int min_pts,
                         int pts_in_cell, int small_max, int32_t* rows, int32_t* cols,
                         int64_t* nblocks, int64_t* m);
/* begin with separate partition keys (getClusterFromList); share / cluster / finish are unchanged */
int vcp_blocks_begin_keyed(vcp_ctx* ctx, const double* key_xy, const double* motor, int64_t n, double eps,
                           int min_pts, int pts_in_cell, int small_max, int32_t* rows, int32_t* cols,
                           int64_t* nblocks, int64_t* m);
int vcp_blocks_begin_keyed_dev(vcp_ctx* ctx, const double* d_key_xy, const double* d_motor, int64_t n, double eps,
                               int min_pts, int pts_in_cell, int small_max, int32_t* rows, int32_t* cols,
                               int64_t* nblocks, int64_t* m);
int vcp_blocks_share(vcp_ctx* ctx, int rank, int world, int32_t* block_lo, int32_t* block_hi,
                     int64_t* pos_lo, int64_t* pos_hi);
int vcp_blocks_cluster_dev(vcp_ctx* ctx, int32_t block_lo, int32_t block_hi, int32_t* d_local,
                           int64_t* evals);
int vcp_blocks_finish_dev(vcp_ctx* ctx, const int32_t* d_local, int64_t evals_blocks,
                          int32_t* d_labels, int32_t* d_block_of, int64_t* d_merge_order,
                          int64_t* m_out, int32_t* kept, int32_t* del_sum, int32_t* cluster_amount,
                          int64_t* dist_evals);

/* The same pipeline with EVERY stage sharded (one process and one context per GPU; every rank holds the cloud, or at
 * least can read it): the ranks repeat only the streaming passes that decide the partition, build, cluster and merge
 * their own share of the blocks, and exchange a few words plus the final (index, label) pairs -- driver:
 * vtkcloudpoint_amd/distributed.py: sharded_pipeline; result = vcp_dbscan_blocks, bit for bit.
 *   plan      bounds, first block (FrmMain.cs:1224-1258), block of every point and the population of every SUPER-BUCKET
 *             (2^k consecutive block ids, *nsuper of them): identical on every rank
 *   cuts      cuts [world + 1]: first super-bucket of every rank, balanced on the point count (host arithmetic)
 *   build     the block-major list of the super-buckets [super_lo, super_hi) only (:1259-1285): blocks
 *             [*block_lo, *block_hi), *m_loc points in them, *n_loc points in all (the last share also holds the
 *             points in no block)
 *   cluster   vcp_blocks_cluster_dev on [*block_lo, *block_hi), d_local [m_loc]
 *   local     CompleteWork3 inside the share (:1442-1504): info = {clusters, kept ones, error (the C# would throw),
 *             request (the demotion quirk of :1485-1488 reaches the last entry of an EARLIER share), the share has a
 *             non-empty block, its last entry still carries a label, m_loc, n_loc}
 *   -- exchange: kept offsets; whose last entry is zeroed (the nearest earlier share with a non-empty block) --
 *   zero      zero_last != 0: zero that entry; the zero list of the share (:1510-1515): *z_count points, of which
 *             *active_count can be reached by the noise pass at all -- those within 2 eps of their block's boundary and
 *             those that lost a label (csrc/blocks.hip: k_zero_flag); everybody else provably keeps 0
 *   zcoords   the active points' coordinates [active_count * 2] in zero-list order (swap_xy: as (y, x); shares are bands
 *             in y)
 *   -- the global noise pass over all shares' active points: vcp_slab_* (exact DBSCAN over several GPUs), cf preset;
 *      DBImproved.iritatorNum of the pass = Z x (Z + clusters + border points queried twice), Z = sum of z_count --
 *   pairs     d_pairs [n_loc] = (original index << 32 | final label): kept clusters + kept_offset, active points with
 *             d_zlab [active_count] (their labels from the noise pass), everybody else 0
 *   scatter   d_labels[index] = label for count pairs (any rank's), indices < n */
int vcp_blocks_plan_dev(vcp_ctx* ctx, const double* d_key_xy, const double* d_motor, int64_t n, double eps, int min_pts,
                        int pts_in_cell, int small_max, int32_t* rows, int32_t* cols, int64_t* nblocks, int64_t* nsuper);
int vcp_blocks_plan_cuts(vcp_ctx* ctx, int world, int64_t* cuts);
int vcp_blocks_build_dev(vcp_ctx* ctx, int64_t super_lo, int64_t super_hi, int32_t* block_lo, int32_t* block_hi,
                         int64_t* m_loc, int64_t* n_loc);
int vcp_blocks_finish_local_dev(vcp_ctx* ctx, const int32_t* d_local, int64_t info[8]);
int vcp_blocks_finish_zero_dev(vcp_ctx* ctx, int zero_last, int64_t* z_count, int64_t* active_count);
int vcp_blocks_finish_zcoords_dev(vcp_ctx* ctx, int swap_xy, double* d_zcoords);
int vcp_blocks_finish_pairs_dev(vcp_ctx* ctx, int32_t kept_offset, const int32_t* d_zlab, int64_t* d_pairs);
int vcp_scatter_pairs_dev(vcp_ctx* ctx, const int64_t* d_pairs, int64_t count, int64_t n, int32_t* d_labels);

/* -- several GPUs from ONE process -----------------------------------------------------------
 * The reference fans its blocks out from one process (ThreadPool.QueueUserWorkItem(StartCode, cells[i]) per block,
 * FrmMain.cs:1356-1359) and merges on the UI thread (CompleteWork3, :1442-1520).  vcp_multi is the drop-in form of
 * that for a host that owns several GPUs: one vcp_ctx per listed HIP device (a device id may repeat: several contexts
 * on one GPU), driven by one host thread each.  vcp_dbscan_blocks_multi = vcp_dbscan_blocks_keyed (key_xy may be NULL)
 * with every stage sharded (round 3): each device repeats the streaming passes that decide the partition, then builds,
 * clusters and merges its own share of the blocks (the vcp_blocks_plan_dev ... stages below); the shares' counters meet
 * in this process's memory, the active points of the zero lists travel to device 0 as peer copies over xGMI, device 0
 * runs the global noise pass over them and assembles the label array from the devices' (index, label) pairs.  Results
 * are identical to the one-device call, bit for bit.  (The multi-PROCESS form -- one rank per GPU, RCCL all-gathers -- is
 * vtkcloudpoint_amd/distributed.py: sharded_pipeline, over the same stages.) */
typedef struct vcp_multi vcp_multi;
int vcp_create_multi(const int* device_ids, int n, vcp_multi** out);
void vcp_destroy_multi(vcp_multi* m);
const char* vcp_multi_last_error(const vcp_multi* m); /* m may be NULL: last create error */
int vcp_multi_count(const vcp_multi* m);
vcp_ctx* vcp_multi_ctx(vcp_multi* m, int i);          /* borrowed: context of device i for single-GPU calls */
int vcp_dbscan_blocks_multi(vcp_multi* m, const double* key_xy, const double* motor, int64_t n, double eps, int min_pts,
                            int pts_in_cell, int small_max, int32_t* labels, int32_t* block_of, int64_t* merge_order,
                            int64_t* m_out, int32_t* rows, int32_t* cols, int32_t* kept, int32_t* del_sum,
                            int32_t* cluster_amount, int64_t* dist_evals);
/* The range arithmetic of vcp_blocks_share and vcp_dbscan_blocks_multi as a pure host function (no device, no
 * context): blockstart [nblocks + 1] = first block-major position of every block (ascending, blockstart[nblocks] = m);
 * cuts [world + 1] <- first block of every rank (cuts[0] = 0, cuts[world] = nblocks): rank r starts at the first block
 * whose first position is >= m * r / world. */
int vcp_blocks_share_plan(const uint32_t* blockstart, int64_t nblocks, int world, int64_t* cuts);

/* -- exact DBSCAN over several GPUs (SURVEY.md 8e mode 2) -----------------------------------
 * One monolithic DBImproved.dbscan (BC/DBImproved.cs:91-114) over a cloud that is spread over several
 * ranks (one process and one context per GPU): every rank clusters its own points plus a 2*eps halo of
 * the other ranks' points, the ranks agree on the components that cross a boundary, and each labels its
 * own points with the ids the single-GPU call would have produced (vtkcloudpoint_amd/distributed.py:
 * exact_slabs drives the exchange over RCCL).
 *   begin    d_coords [n*dim] = own points followed by halo points; d_ord [n] = position of each point in
 *            the GLOBAL list (what "index in lst" means for the seed / numbering rules); d_noexpand [n]
 *            (may be NULL) = 1 for points whose neighbourhood is incomplete here: they count as
 *            neighbours but never seed or extend a cluster.  Builds the grid, the core flags and the
 *            LOCAL components; writes d_rep [n] = smallest ord of the point's local component
 *            (0xFFFFFFFF for points that are not expanding) and d_is_core [n] (may be NULL);
 *            *n_comp = number of local components.
 *   comps    copies the n_comp component seeds (their smallest ord, in no particular order) to the host.
 *   finish   map_rep [n_comp] strictly ascending = the component seeds; map_k [n_comp] = index of the
 *            component's GLOBAL cluster in the table tab_gid / tab_seed [n_tab] (cluster id, strictly
 *            ascending, and the global seed position of that cluster); all four are host arrays.  Applies
 *            the border rule (:87, largest adjacent id) and writes d_labels [n], d_is_classed [n] (may be
 *            NULL); *twice = own points (own_lo <= ord < own_lo + own_count) that the C# loop queries a
 *            second time (the iritatorNum term).
 * The state lives in the context's workspace: no other call on this context between begin and finish, and d_coords
 * (read in place by the exact re-tests of the finish stage too) stays valid and unchanged until finish has returned. */
int vcp_slab_begin(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, double eps,
                   int min_pts, const uint8_t* d_noexpand, const uint32_t* d_ord, uint32_t* d_rep,
                   uint8_t* d_is_core, int64_t* n_comp);
int vcp_slab_comps(vcp_ctx* ctx, uint32_t* comp_rep);
int vcp_slab_finish(vcp_ctx* ctx, const uint32_t* map_rep, const uint32_t* map_k, int64_t n_tab,
                    const int32_t* tab_gid, const uint32_t* tab_seed, uint32_t own_lo, uint32_t own_count,
                    int32_t* d_labels, uint8_t* d_is_classed, int64_t* twice);

/* -- centroids ----------------------------------------------------------------------------
 * Replaces Tools.GetClusList (BC/Tools.cs:162-195; also getClusterCenter :118-155): per cluster
 * id 1..K the mean of (X,Y,Z) -> c3 [K*3] and of (motor_x,motor_y) -> c2 [K*2]; counts [K].
 * xyz or motor may be NULL (then c3 / c2 is not written).  Empty clusters: count 0, NaN rows.
 * Sums are fixed-order binary64 tree reductions (run-to-run deterministic; they differ from the
 * C#'s sequential sum in the last bits -- tolerance 1e-12 relative). */
int vcp_centroids(vcp_ctx* ctx, const double* xyz, const double* motor, const int32_t* labels,
                  int64_t n, int32_t K, double* c3, double* c2, int64_t* counts);
int vcp_centroids_dev(vcp_ctx* ctx, const double* d_xyz, const double* d_motor, const int32_t* d_labels,
                      int64_t n, int32_t K, double* d_c3, double* d_c2, int64_t* d_counts);

/* Replaces Tools.getFixedPtsCentroid(clusList, isIgnoreDuplication) (BC/Tools.cs:78-111; caller
 * SureDistanceFilter.cs:74): per list 1..K the ptsCount-weighted mean of (X,Y,Z).  group [n] = which ClusObj.li the
 * point sits in (1..K, 0 = none); cluster_id [n] = Point3D.clusterId (NULL = group); pts_count [n] = Point3D.ptsCount
 * (FrmMain.cs:1074,1081: multiplicity of a deduplicated fixed point).  A member with clusterId != 0 counts ONCE when
 * ignore_duplication is set, otherwise ptsCount times (:88-101).  c3 [K*3]; inside_num [K] (may be NULL) = the C#'s
 * insideNum (0 gives NaN rows, 0/0).  An empty list makes the C# throw at li[0] (:106): VCP_ERR_INDEX.
 * Sums are the fixed tree of vcp_centroids (1e-12 relative to the C#'s sequential sum). */
int vcp_centroids_weighted(vcp_ctx* ctx, const double* xyz, const int32_t* group, const int32_t* cluster_id,
                           const int32_t* pts_count, int64_t n, int32_t K, int ignore_duplication, double* c3,
                           int64_t* inside_num);

/* Replaces Tools.MergeIDByDistance (BC/Tools.cs:580-621): DBImproved(minPts 2, L1 on X,Y) over the
 * K centroids; map_to[k] = cluster id the k-th centroid's cluster is merged into, 0 = none. */
int vcp_merge_centroids(vcp_ctx* ctx, const double* cxy, const int32_t* ids, int32_t K, double thr,
                        int32_t* map_to, int32_t* merge_count);
/* Replaces Tools.refreshCensAndClusByDictionary (BC/Tools.cs:521-572): relabel points through
 * map_by_id (index id-1, 0 = keep), renumber surviving ids 1..K' ascending, recompute centroids. */
int vcp_refresh_by_dictionary(vcp_ctx* ctx, const double* xyz, const double* motor, int32_t* labels,
                              int64_t n, int32_t K, const int32_t* map_by_id, int32_t* new_k,
                              double* c3, double* c2, int64_t* counts);

/* -- ICP ------------------------------------------------------------------------------------
 * Replaces ICP.go_hell_ICP(model, data, R, T, e) (BC/ICP.cs:18-181): per round nearest model
 * point per data point (FindClosestPointSet :224-250, lowest index on ties), the 16 sums
 * (CalculateMeanPoint3D :255-273, sum p y^T :38-52, SSE :126-133), Horn's closed form on the
 * host (the INTENDED arithmetic of :53-124; the as-written code is non-functional, SURVEY.md
 * fact 4), composition R <- R1 R, T <- R1 T + T1 (:149-177), P <- R data + T (TransPoint
 * :195-219).  model [nm*3], data [nd*3]; R [9] row-major and T [3] are outputs. */
int vcp_icp(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, double tol,
            int max_iter, int stop_rule, double R[9], double T[3], double* sse, double* rmse,
            int32_t* iters);
int vcp_icp_dev(vcp_ctx* ctx, const double* d_model, int64_t nm, const double* d_data, int64_t nd,
                double tol, int max_iter, int stop_rule, double R[9], double T[3], double* sse,
                double* rmse, int32_t* iters);
/* One correspondence pass (A10+A11): sums[16] = sum p[3], sum y[3], sum p y^T[9], SSE for
 * p = R data + T; nn [nd] may be NULL.  R,T NULL = identity.
 * The summation order -- and with it every bit of sums[] -- is fixed by (nm, nd, whether every model coordinate is
 * finite) and by nothing else: not by the device, the context's history or nn being NULL.  The order is restated in
 * tests/icp_sums_ref.py (a numpy replay the suite compares with bit for bit) and in DESIGN.md section 13. */
int vcp_icp_sums(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                 const double R[9], const double T[3], double sums[16], int32_t* nn);

/* "VTK-like" ICP: the configuration MainForm.ICP() gives VTK's closed
 * vtkIterativeClosestPointTransform (FrmMain.cs:851-862), behaviour per the VTK 5.0 header
 * (vtkIterativeClosestPointTransform.h:49-180): landmarks = every step-th source point (step = ns /
 * max_landmarks when ns > max_landmarks; VTK's default cap is 200), optional start by matching centroids,
 * exactly max_iter rounds (the reference sets 100 and leaves the mean-distance check off), rigid body.
 * source [ns*3] (the reference feeds (tmp_X, tmp_Y, 0), Tools.cs:696-703), target [nt*3]; M = the accumulated
 * 4x4 row-major matrix (what icp.GetMatrix() returns, FrmMain.cs:862); mean_dist = RMS landmark-to-closest
 * distance seen by the last round.  PARITY UNPINNED against VTK itself (sources not in the reference tree). */
int vcp_icp_vtklike(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                    int max_iter, int max_landmarks, int start_by_matching_centroids, double M[16],
                    double* mean_dist, int32_t* iters);

/* -- multi-start ICP ----------------------------------------------------------------------------
 * vcp_icp_vtklike falls into a local minimum on checkerboard-like truths (the reference's README, "bugs known"; its
 * workaround is a hand-placed start, FrmMain.cs:3471-3537, and typed axis directions, :912-913).  This runs the
 * vcp_icp_vtklike loop from n_poses starts in one call, scores each result and keeps the best:
 *   per pose h     the vcp_icp_vtklike loop with start_by_matching_centroids on -- the same landmarks (step = ns /
 *                  max_landmarks when ns > max_landmarks), exactly max_iter rounds, the same NN, sums, Horn solve and
 *                  composition R <- R1 R, T <- R1 T + T1, the same mean_dist (RMS landmark-to-closest distance of the
 *                  last round) -- from R = R0_h, T = T0_h
 *   init_R         [n_poses*9] row-major, used as given; a reflection (det -1) is allowed and kept (Horn's R1 is
 *                  proper): that covers an unknown axis direction.  NULL: R0_h = Rz(theta_h) = [[c,-s,0],[s,c,0],
 *                  [0,0,1]], theta_h = h * (2 pi / n_poses) in binary64, c = cos, s = sin of the C library; h = 0 is
 *                  exactly the identity
 *   init_T         [n_poses*3].  NULL: T0_h = mt - R0_h ms, with ms, mt the source and target means computed as
 *                  vcp_icp_vtklike does (sequential binary64 sums over all points, one division) and R0_h ms row by
 *                  row, left to right -- for R0 = I bit-identical to vcp_icp_vtklike's start
 *   inliers[h]     over ALL ns source points under M_h = [R_h | T_h]: points whose nearest target is closer than
 *                  inlier_dist, by vcp_match's arithmetic and rule, so inliers[h] == vcp_match(source, target, M_h,
 *                  inlier_dist).count_matched; inlier_dist = +inf is allowed
 *   best           the pose with the most inliers; ties go to the smaller mean_dist, then to the lower h.  M_best =
 *                  its 4x4 row-major matrix, laid out like vcp_icp_vtklike's M
 *   M_all [n_poses*16], mean_dist [n_poses], inliers [n_poses] may each be NULL; M_best and best are required.
 * The result of pose h is bit-identical whatever other poses share the call: each pose's partition into workgroups and
 * reduction order are those of a single run.  n_poses = 1 with init_R = init_T = NULL equals vcp_icp_vtklike
 * (start_by_matching_centroids = 1) bit for bit (M, mean_dist).  Errors: those of vcp_icp_vtklike; n_poses < 1,
 * inlier_dist NaN or <= 0, a non-finite entry of init_R / init_T: VCP_ERR_ARG; n_poses > 4096: VCP_ERR_UNSUPPORTED; a
 * failed Horn solve in any pose: VCP_ERR_ARG.  Deterministic.  Timing phases: icpms_rounds, icpms_score
 * (csrc/icp.hip). */
int vcp_icp_multistart(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                       int32_t n_poses, const double* init_R, const double* init_T, int max_iter,
                       int max_landmarks, double inlier_dist, double M_best[16], int32_t* best,
                       double* M_all, double* mean_dist, int32_t* inliers);

/* -- gated ICP ------------------------------------------------------------------------------------
 * Every loop above feeds every landmark into the round's 16 sums, however far its nearest target is; centroid lists
 * hold false clusters (a wall beside the target field, clutter between targets) that pull every round.  The gated
 * forms leave pairs beyond a per-round distance out of the sums (PCL's setMaxCorrespondenceDistance, Open3D's
 * max_correspondence_distance; VTK's class has none).
 *
 * One round, state (R, T), gate g.  The landmark p = R d + T and its nearest target y are those of vcp_icp_sums: the
 * same transform, the same NN rule, lowest index on ties.  With e = p - y,
 *   dd = e0*e0 + e1*e1 + e2*e2     the SSE term: binary64, left to right, no contraction
 *   the pair is DROPPED iff sqrt(dd) >= g (correctly rounded sqrt).  A NaN dd is kept and poisons the sums, as it
 *   does ungated; with finite coordinates that do not overflow, g = +inf drops nothing.
 * A dropped pair adds +0.0 to each of the 16 sums AT ITS OWN PLACE in vcp_icp_sums's summation order, which stays fixed
 * by (nm, nd, whether every model coordinate is finite) and nothing else: tests/icp_sums_ref.py replays it with the
 * dropped rows zeroed.  kept = the exact number of kept pairs.  The round's Horn step is the ungated one on (sums,
 * kept): kept takes the place of nd, the eigenvector basis is carried from round to round as before.  A round with
 * kept < min_pairs is STARVED: R, T and the basis stay as they are, the round still counts, and `starved` goes up by
 * one.  mean_dist of a round = sqrt(sums[15] / kept), +inf when kept = 0.
 *
 * vcp_icp_sums_gated: one gated pass, the test handle on the kernels as vcp_icp_sums is.  Arguments as vcp_icp_sums;
 * *kept (required) = the count; nn [nd] and keep [nd] (1 = kept, 0 = dropped) may be NULL.  gate NaN or <= 0:
 * VCP_ERR_ARG, nothing written.  gate = +inf: sums bit-identical to vcp_icp_sums.
 *
 * vcp_icp_gated: vcp_icp_multistart with a gate schedule.  Everything not named here is vcp_icp_multistart's, word for
 * word: the landmarks, the default poses and starts, exactly max_iter rounds, the composition, the inlier score over
 * all ns source points (not gated: inlier_dist alone decides it), best = most inliers, then the smaller mean_dist,
 * then the lower h.
 *   gates [n_gates]  round r (1-based) uses gates[min(r, n_gates) - 1]: the last entry serves every later round
 *   min_pairs        the fewest kept pairs a round acts on (3 determines a rigid motion of points in general position)
 *   kept [n_poses]   the last round's count; starved [n_poses] the number of starved rounds.  Both may be NULL.
 * n_gates < 1, min_pairs < 1, a gate NaN or <= 0: VCP_ERR_ARG.  A failed Horn solve in a round that is not starved:
 * VCP_ERR_ARG, as in vcp_icp_multistart.  No output is written on an error.  The other errors and limits are
 * vcp_icp_multistart's.  With every gate +inf, M_all, mean_dist, inliers and best equal vcp_icp_multistart's bit for
 * bit, kept is the landmark count and starved 0.  A pose's bits do not depend on the other poses of the call.  The
 * schedule is read on the device: all rounds are enqueued at once, one synchronisation at the end.
 * Timing phases: icpg_rounds, icpg_score (csrc/icp.hip). */
int vcp_icp_sums_gated(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                       const double R[9], const double T[3], double gate, double sums[16], int64_t* kept,
                       int32_t* nn, uint8_t* keep);
int vcp_icp_gated(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                  int32_t n_poses, const double* init_R, const double* init_T, int max_iter, int max_landmarks,
                  const double* gates, int32_t n_gates, int32_t min_pairs, double inlier_dist, double M_best[16],
                  int32_t* best, double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept,
                  int32_t* starved);

/* -- trimmed ICP -----------------------------------------------------------------------------------
 * A gate is a distance: to set its schedule the caller has to know the start error, the centroid noise and the unit of
 * the scan before a pose exists.  What the caller does know is a SHARE: with T truths, K centroids and `visible` the
 * fraction of the truths the scan is expected to see, about min(1, visible T / K) of the centroids are real targets.
 * Trimmed ICP (Chetverikov et al. 2002) takes that share: every round fits on the m pairs with the smallest distances
 * and leaves the rest out.  It is unit-free (scaling every coordinate by a power of two scales the translation and
 * changes nothing else) and cannot starve from a bad start the way a closed gate does.
 *
 * One round, state (R, T), keep count m with 1 <= m <= L, L the number of landmarks of the call (nd for the one-pass
 * handle).
 *   Pair and distance: vcp_icp_sums's.  p = R d + T, the nearest target y with the lowest index on ties, e = p - y,
 *     dd = e0*e0 + e1*e1 + e2*e2    the SSE term: binary64, left to right, no contraction.
 *   Key: landmark i (its position in the landmark list, 0-based) has the 96-bit key [K(dd) | i], K(dd) = the bit
 *     pattern of dd as a uint64 when dd is not NaN, 0xFFFFFFFFFFFFFFFF when it is.  A non-NaN dd is >= +0, so the
 *     unsigned order is the numeric order; +inf ranks before NaN, NaN ranks last.  Keys are distinct: equal distances go
 *     to the lower landmark index.
 *   Kept: the m pairs with the smallest keys.  Every other pair is DROPPED and adds +0.0 to each of the 16 sums AT ITS
 *     OWN PLACE in vcp_icp_sums's summation order, which stays fixed by (nm, nd, whether every model coordinate is finite)
 *     and nothing else.  A kept NaN poisons the sums as it does ungated; it is kept only when m reaches it.
 *   thr: the dd of the kept pair with the largest key.  trim_dist = sqrt(thr), correctly rounded: the gate this round
 *     was equivalent to.
 *   Step: the gated step on (sums, kept = m): kept takes the place of nd, the basis is carried.  A round with
 *     m < min_pairs is STARVED: R, T and the basis stay, the round still counts, `starved` goes up by one.
 *     mean_dist = sqrt(sums[15] / kept).
 *
 * vcp_icp_sums_trimmed: one trimmed round's passes, the test handle as vcp_icp_sums_gated is.  *thr_dd (required) = thr;
 * nn [nd] and keep [nd] (1 = kept, 0 = dropped) may be NULL.  m < 1 or m > nd: VCP_ERR_ARG, nothing written.  m = nd:
 * sums bit-identical to vcp_icp_sums.  The key holds the landmark in 32 bits: nd >= 2^32 is VCP_ERR_TOO_LARGE.
 *
 * vcp_icp_trimmed: vcp_icp_multistart with a keep schedule.  Arguments as vcp_icp_gated, with keep [n_keep] in place of
 * gates [n_gates] and one more optional output, trim_dist [n_poses], the last round's value (that of a starved round
 * too: the select runs in every round).
 *   keep [n_keep]   round r (1-based) uses f = keep[min(r, n_keep) - 1] and m = min(L, (int64_t)ceil(f * (double)L)):
 *                   one multiplication, the ceiling is exact
 * n_keep < 1, min_pairs < 1, an entry that is NaN, <= 0 or > 1: VCP_ERR_ARG.  A failed Horn solve in a round that is
 * not starved: VCP_ERR_ARG.  No output is written on an error.  All other errors and limits are vcp_icp_multistart's.
 * Everything not named here is vcp_icp_multistart's, word for word: the landmarks, the default poses and starts,
 * exactly max_iter rounds, the composition, the inlier score over all ns source points (not trimmed), the choice of
 * the best pose.  With every entry 1.0, M_all, mean_dist, inliers and best equal vcp_icp_multistart's bit for bit,
 * kept = L and starved = 0.  A pose's bits do not depend on the other poses of the call.  The schedule is read on the
 * device: all rounds are enqueued at once, one synchronisation at the end.  Deterministic: only integer comparisons
 * and integer atomics decide the selection.  The select is a most-significant-digit radix select over the 96-bit keys,
 * 8 bits a digit: up to VCP_ICPT_SELECT_WG_MAX landmarks one workgroup per pose holds the keys in LDS (one launch per
 * round), beyond that a histogram kernel runs once per digit over many workgroups (13 launches per round, whatever
 * the data).  Extra workspace: 12 bytes per (pose, landmark) -- the 8-byte K(dd) and the 4-byte index found -- and
 * 12 480 bytes per pose for the larger form's prefixes and histograms; no new size limit beyond VCP_ERR_NOMEM.
 * Timing phases: icpt_rounds, icpt_score (csrc/icp.hip). */
#define VCP_ICPT_SELECT_WG_MAX 4096
int vcp_icp_sums_trimmed(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                         const double R[9], const double T[3], int64_t m, double sums[16], double* thr_dd,
                         int32_t* nn, uint8_t* keep);
int vcp_icp_trimmed(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                    int32_t n_poses, const double* init_R, const double* init_T, int max_iter, int max_landmarks,
                    const double* keep, int32_t n_keep, int32_t min_pairs, double inlier_dist, double M_best[16],
                    int32_t* best, double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept,
                    int32_t* starved, double* trim_dist);

/* -- similarity ICP --------------------------------------------------------------------------------
 * Every form above composes proper rotations onto the start: a start whose scale is off (centroids in another unit
 * than the truths, vcp_register_sim's k from one pair per base) keeps that error, and an error of 2 % moves the edge of
 * a 20 x 20 field by more than a closed gate of 0.1.  This form is the gated loop whose round fits rotation, translation
 * and ONE isotropic scale (vtkLandmarkTransform's Similarity mode; Horn 1987, section 2.E, the symmetric scale).
 * Everything is binary64, each operation rounded on its own, sqrt and / correctly rounded.
 *
 * Pass.  vcp_icp_sums_gated's, with two more columns.  For a kept pair, p = R d + T and y its nearest model point:
 *   sums[16] += (p0*p0 + p1*p1) + p2*p2        sums[17] += (y0*y0 + y1*y1) + y2*y2
 * A dropped pair adds +0.0 to both at its own place; a kept NaN poisons them.  Both go through the SAME summation tree
 * as the sixteen, fixed by (nm, nd, whether every model coordinate is finite); sums[0..15] are bit-identical to
 * vcp_icp_sums_gated's at the same gate.
 *
 * Step, on (sums [18], n = kept, c = the product of the factors applied so far, bounds ratio_min <= ratio_max).
 *   R1, muP, muY: vcp_selftest_horn's on sums[0..15], basis handling included.  Where that fails, this fails.
 *   N = (double)n;  vP = sums[16]/N - ((muP0*muP0 + muP1*muP1) + muP2*muP2);  vY likewise from sums[17] and muY.
 *   The scale is DETERMINED iff 0 < vP < inf and 0 < vY < inf (comparisons with NaN are false).  Then
 *     k = sqrt(vY / vP), t = c * k;
 *     t < ratio_min: c_new = ratio_min, k_used = ratio_min / c;  t > ratio_max: c_new = ratio_max, k_used = ratio_max / c;
 *     otherwise c_new = t, k_used = k.
 *   Not determined (coincident points, every pair on one target, cancellation far from the origin): k_used = 1.0,
 *     c_new = c.  Not fatal.
 *   R1s[j] = k_used * R1[j];  T1[i] = muY[i] - (R1s[3i]*muP0 + R1s[3i+1]*muP1 + R1s[3i+2]*muP2).
 *   Where k_used == 1.0, R1s and T1 are the rigid step's bit for bit.  The step is exactly invariant under a
 *   power-of-two scaling of all coordinates (k_used, R1s and the return value bit-identical, T1 scaled) while nothing
 *   leaves the normal range.  Accuracy of k: DESIGN.md section 22.
 *
 * vcp_icp_sums_sim: one pass, the test handle.  Arguments, drop rule, kept, nn, keep and errors are
 * vcp_icp_sums_gated's; sums has 18 entries.  gate = +inf is the ungated pass.
 *
 * vcp_selftest_horn_sim: the step on the host, compiled from the source the device runs; needs no device.  Returns 1
 * (scale determined), 2 (not determined), 0 (the Horn solve failed: nothing but V written, as vcp_selftest_horn) or
 * VCP_ERR_ARG: a NULL pointer, n <= 0, use_v without V, c NaN or <= 0, ratio_min NaN or <= 0, ratio_max NaN, +inf or
 * < ratio_min.
 *
 * vcp_icp_sim: vcp_icp_gated with that step.  Everything not named here is vcp_icp_gated's, word for word: the
 * landmarks, the default poses and starts, exactly max_iter rounds, the starved rule, the composition R <- R1s R,
 * T <- R1s T + T1, the score over all ns points, the choice of the best pose, no output on an error, a pose's bits
 * independent of the other poses, all rounds enqueued at once with one synchronisation.
 *   Every pose carries c, 1.0 at the start; a round that is not starved runs the step on (sums, kept, c).
 *   ratio [n_poses]     (may be NULL) the final c: the nominal product of the applied factors.  The pose's actual scale is
 *                       sqrt|det| of its planar block; it differs from c times the start's scale by roundings only.
 *   unscaled [n_poses]  (may be NULL) the number of rounds whose scale was not determined.
 * VCP_ERR_ARG also for ratio_min NaN or <= 0, ratio_max NaN, +inf or < ratio_min, and unless ratio_min <= 1 <= ratio_max.
 * A failed Horn solve in a round that is not starved: VCP_ERR_ARG.  With ratio_min == ratio_max == 1.0 every factor is
 * 1.0 / 1.0: M_all, mean_dist, inliers, best, kept and starved equal vcp_icp_gated's bit for bit and ratio is 1.0.
 * Timing phases: icps_rounds, icps_score (csrc/icp.hip). */
int vcp_icp_sums_sim(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                     const double R[9], const double T[3], double gate, double sums[18], int64_t* kept, int32_t* nn,
                     uint8_t* keep);
int vcp_selftest_horn_sim(const double sums[18], int64_t n, double V[16], int use_v, double c, double ratio_min,
                          double ratio_max, double R1s[9], double T1[3], double* k_used, double* c_new);
int vcp_icp_sim(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                int32_t n_gates, int32_t min_pairs, double ratio_min, double ratio_max, double inlier_dist,
                double M_best[16], int32_t* best, double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept,
                int32_t* starved, double* ratio, int32_t* unscaled);

/* -- unique-correspondence ICP -----------------------------------------------------------------------
 * Every loop above pairs each landmark with its nearest target on its own, so two centroids may fit against one truth.
 * A target produces one centroid: where DBSCAN splits a target, or a reflection or an edge return makes a second
 * cluster beside it, one of the two is a ghost.  A gate cannot remove it (it lies inside any gate that still admits the
 * real centroids' start error) and a trim share does not know that its truth is taken.  This form lets every target
 * take ONE landmark per round, the closest (Zinsser et al. 2003, "picky ICP"); vcp_match_unique does the same at the
 * end of the pipeline.
 *
 * One round, state (R, T), gate g.
 *   Pair and distance: vcp_icp_sums's.  p = R d + T, the nearest target y with the lowest index on ties, e = p - y,
 *     dd = e0*e0 + e1*e1 + e2*e2    the SSE term: binary64, left to right, no contraction.
 *   Key: the trimmed form's.  Landmark i (its position in the landmark list, 0-based) has the 96-bit key [K(dd) | i],
 *     K(dd) = the bit pattern of dd as a uint64 when dd is not NaN, 0xFFFFFFFFFFFFFFFF when it is.
 *   Winner: the WINNER of target j is the landmark with the smallest key among all landmarks whose nearest target is j.
 *     The gate plays no part in this choice: a winner the gate drops does not hand its target to the next landmark.
 *   Kept: a landmark is KEPT iff it is its target's winner and the gate does not drop it; the gate drops iff
 *     sqrt(dd) >= g, as in vcp_icp_sums_gated.  A NaN dd wins only where every pair of that target is NaN; it is then
 *     kept and poisons the sums, as it does ungated.  Every other pair adds +0.0 to each of the 16 sums AT ITS OWN PLACE
 *     in vcp_icp_sums's summation order, which stays fixed by (nm, nd, whether every model coordinate is finite) and
 *     nothing else.
 *   kept = the number of kept pairs.  lost = the number of pairs that are not their target's winner, whatever the gate
 *     says of them.
 *   Step, starved rule, basis carry, composition, mean_dist (= sqrt(sums[15] / kept), +inf at kept = 0), score and the
 *     choice of the best pose: vcp_icp_gated's, word for word.
 *
 * vcp_icp_sums_unique: one round's passes, the test handle as vcp_icp_sums_gated is.  Arguments as vcp_icp_sums_gated,
 * then *lost (required).  keep [nd] (may be NULL): 2 = not the winner, 0 = winner dropped by the gate, 1 = kept.
 * Errors are vcp_icp_sums_gated's; a NULL lost is VCP_ERR_ARG; the key holds the landmark in 32 bits: nd >= 2^32 is
 * VCP_ERR_TOO_LARGE.  With gate = +inf and an nn that is injective on the data, sums are bit-identical to vcp_icp_sums.
 *
 * vcp_icp_unique: vcp_icp_gated with that rule.  Arguments as vcp_icp_gated, then lost [n_poses] (may be NULL), the
 * last round's count.  Errors and limits are vcp_icp_gated's; no output is written on an error.  Where nn is injective
 * on the landmarks in every round, M_all, mean_dist, inliers, best, kept and starved equal vcp_icp_gated's bit for bit
 * and lost is 0.  Deterministic: only integer comparisons and integer atomics decide the selection (a 64-bit minimum of
 * K(dd) per target, then a 32-bit minimum of the landmark among the ties); two calls give identical bits, and a pose's
 * bits do not depend on the other poses of the call.  The schedule is read on the device: all rounds are enqueued at
 * once, one synchronisation at the end.  Extra workspace: 12 bytes per (pose, landmark) and 12 bytes per
 * (pose, target) -- the slot of that target, all ones between rounds: filled once per call, and after every round only
 * the slots that round's landmarks touched are set back, so a round's cost does not grow with nt beyond the NN search.
 * No new size limit beyond VCP_ERR_NOMEM.
 * Timing phases: icpu_rounds, icpu_score (csrc/icp.hip). */
int vcp_icp_sums_unique(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                        const double R[9], const double T[3], double gate, double sums[16], int64_t* kept,
                        int32_t* nn, uint8_t* keep, int64_t* lost);
int vcp_icp_unique(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                   int32_t n_poses, const double* init_R, const double* init_T, int max_iter, int max_landmarks,
                   const double* gates, int32_t n_gates, int32_t min_pairs, double inlier_dist, double M_best[16],
                   int32_t* best, double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept,
                   int32_t* starved, int64_t* lost);

/* -- anisotropic ICP --------------------------------------------------------------------------------
 * The reference puts the centroids into the truths' unit with TWO factors, scale[0] for X and scale[1] for Y
 * (FrmMain.cs:3046-3055: the motor's two axes do not have the same gain), taken from two bounding boxes, and only then
 * runs the rigid loop.  The similarity form fits one factor for both.  This form is the gated loop whose round fits a
 * rotation, a translation and one scale per axis: the pose sought is y = R diag(sx, sy, 1) d + t.  z keeps scale 1: the
 * reference's input is planar (Tools.cs:696-703) and a free z-scale would be undetermined there.
 * Every other form works in the transformed frame and composes a small step onto the pose; such a step cannot stay
 * inside R diag(s).  So this form sums over the RAW landmark d, and its step SETS the pose.
 * Everything is binary64, each operation rounded on its own, sums left to right as written, / correctly rounded.
 *
 * Pass.  The pose applied is A (any finite 3x3) and T: p = A d + T, by vcp_icp_sums's TransPoint.  The pair, the
 * distance, dd, the drop rule, kept, nn and keep are vcp_icp_sums_gated's, word for word.  For a kept pair, y its
 * nearest model point:
 *   sums[r] += d_r        sums[3+r] += y_r        sums[6+3r+c] += d_r * y_c        sums[15] += dd (under A, T)
 *   sums[16] += d0*d0     sums[17] += d1*d1
 * A dropped pair adds +0.0 to each column at its own place; all 18 columns go through vcp_icp_sums_sim's tree, fixed by
 * (nm, nd, whether every model coordinate is finite).  With A = identity, T = 0 and finite data sums[0..15] are
 * vcp_icp_sums_gated's bit for bit (1*d + 0*... + 0 is d).
 *
 * Step, on (sums [18], n = kept, the carried basis V, the pose's rotation R, its scales s[2], bounds lo[2] <= hi[2]).
 *   N = (double)n;  muD_a = sums[a]/N;  muY_b = sums[3+b]/N.
 *   For a = 0, 1:
 *     C_ab = sums[6+3a+b]/N - muD_a*muY_b  (b = 0..2);   D_a = sums[16+a]/N - muD_a*muD_a;
 *     g_a = (R[a]*C_a0 + R[3+a]*C_a1) + R[6+a]*C_a2
 *     -- the least-squares scale of axis a for the rotation R is g_a / D_a: the problem separates per axis.
 *     The axis is DETERMINED iff 0 < D_a < inf and 0 < g_a < inf (comparisons with NaN are false).  Then
 *     s'_a = g_a / D_a, clamped to [lo_a, hi_a].  Not determined (all kept d share that coordinate, cancellation far
 *     from the origin, a rotation that has turned the axis round): s'_a = s_a.  Not fatal.
 *   S' = sums[0..15] with S'[a] = s'_a * sums[a] and S'[6+3a+b] = s'_a * sums[6+3a+b] for a = 0, 1.
 *   R_new, T_new: vcp_selftest_horn's R1, T1 on (S', n, V), basis handling included.  Where that fails, this fails.
 *   A_new[3i+a] = R_new[3i+a] * s'_a for a = 0, 1;  A_new[3i+2] = R_new[3i+2].
 *   The step SETS the pose: R <- R_new, s <- s', A <- A_new, T <- T_new; nothing is composed.
 * One scale update and one Horn solve per round: block-coordinate descent interleaved with the re-pairing.  For a fixed
 * kept set neither half-step raises sum |R S d + t - y|^2.  Two exact invariances, while nothing leaves the normal range:
 * scaling every coordinate of data and model by 2^k leaves s', R_new and the return value bit-identical and scales
 * T_new; scaling the data's x alone by 2^k, with s_0, lo_0, hi_0 scaled by 2^-k, leaves R_new, T_new, s'_1 and A_new
 * applied to the scaled data bit-identical and scales s'_0 by 2^-k exactly.  Accuracy of s': DESIGN.md section 25.
 *
 * vcp_icp_sums_aniso: one pass, the test handle.  Arguments and errors are vcp_icp_sums_sim's, A in R's place.
 *
 * vcp_selftest_horn_aniso: the step on the host, compiled from the source the device runs; needs no device.
 * *determined: bit a set = axis a was determined.  Returns 1, 0 (the Horn solve failed: nothing but V written) or
 * VCP_ERR_ARG: a NULL pointer, n <= 0, use_v without V, a NaN or a value <= 0 in s, lo or hi, hi_a = +inf, hi_a < lo_a.
 *
 * vcp_icp_aniso: vcp_icp_gated with that pass and step.  Everything not named here is vcp_icp_gated's, word for word:
 * the landmarks, the default poses, exactly max_iter rounds, the starved rule (pose, scales and basis stay), the score
 * over all ns points, the choice of the best pose, no output on an error, a pose's bits independent of the other
 * poses, all rounds enqueued at once with one synchronisation.
 *   init_scale [n_poses*2]  (may be NULL: all 1.0) the start scales (sx, sy) of every pose
 *   The start of a pose is R = init_R as given, s = init_scale, A[3i+a] = init_R[3i+a]*s_a (a = 0, 1), T = init_T;
 *   where init_T is NULL, T is vcp_icp_gated's centroid start computed with A.  lo_a = ratio_min*init_s_a,
 *   hi_a = ratio_max*init_s_a.  M_all and M_best hold [A | T].
 *   scale [n_poses*2]     (may be NULL) the final (sx, sy)
 *   unscaled [n_poses*2]  (may be NULL) per axis the number of rounds that did not determine it
 * VCP_ERR_ARG also for an init_scale that is NaN, <= 0 or +inf, or whose bound lo_a is 0 or hi_a not finite, and for
 * the ratios by vcp_icp_sim's rules (ratio_min <= 1 <= ratio_max).  A failed Horn solve in a round that is not starved:
 * VCP_ERR_ARG.  With ratio_min == ratio_max == 1.0 the scales never move: the loop is then the rigid fit from A, and it
 * equals vcp_icp_gated from the start A TO ROUNDING ONLY, not bit for bit -- this step sets the pose from sums over d
 * where the gated one composes a step from sums over p.
 * Timing phases: icpa_rounds, icpa_score (csrc/icp.hip). */
int vcp_icp_sums_aniso(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                       const double A[9], const double T[3], double gate, double sums[18], int64_t* kept, int32_t* nn,
                       uint8_t* keep);
int vcp_selftest_horn_aniso(const double sums[18], int64_t n, double V[16], int use_v, const double R[9],
                            const double s[2], const double lo[2], const double hi[2], double R_new[9],
                            double T_new[3], double s_new[2], int32_t* determined);
int vcp_icp_aniso(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                  const double* init_R, const double* init_T, const double* init_scale, int max_iter,
                  int max_landmarks, const double* gates, int32_t n_gates, int32_t min_pairs, double ratio_min,
                  double ratio_max, double inlier_dist, double M_best[16], int32_t* best, double* M_all,
                  double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved, double* scale,
                  int32_t* unscaled);

/* -- congruent-pair global registration ---------------------------------------------------------------
 * Every ICP form above starts from T0 = mean(target) - R0 mean(source) unless told otherwise, which is only right when
 * the scan covers the whole truth field; a scan that sees part of it starts wrong by a large translation from every
 * rotation (the reference's README: ICP "generally relies on RANSAC", which it never wrote).  This call needs no start.
 * Two source points (a base) laid on an ordered pair of targets of the same length give a rigid motion; every such
 * motion is scored by its inliers and the best one per base is kept.  It has no counterpart in the reference.
 * All arithmetic is binary64, every operation rounded on its own, sqrt and / correctly rounded.  The motion is planar: a
 * rotation about z plus a translation (rotations_about_z; the reference feeds (tmp_X, tmp_Y, 0), Tools.cs:696-703).
 *   base        base b is (a, b') = (bases[2b], bases[2b+1]), indices into source; one outside 0..ns-1: VCP_ERR_INDEX
 *   flip        f = 0 always; with mirror != 0, f = 1 too: the source is read as (x, -y, z) throughout
 *   lengths     u = b' - a in (x, y), Lu = sqrt(ux*ux + uy*uy); for ordered targets (i, j), i != j: v = t_j - t_i,
 *               Lv = sqrt(vx*vx + vy*vy).  (b, f, i, j) is a HYPOTHESIS iff 0 < Lu < inf, 0 < Lv < inf and
 *               fabs(Lv - Lu) <= len_tol.  Comparisons with NaN are false: NaN makes no hypothesis
 *   pose        dot = ux*vx + uy*vy, crs = ux*vy - uy*vx, nrm = sqrt(dot*dot + crs*crs); the hypothesis is skipped (it
 *               still counts in n_hyp) unless 0 < nrm < inf.  c = dot/nrm, s = crs/nrm.  Midpoints
 *               ms = ((ax+bx)*0.5, (ay+by)*0.5, (az+bz)*0.5), mt likewise from t_i and t_j.
 *               T = (mt.x - (c*ms.x - s*ms.y), mt.y - (s*ms.x + c*ms.y), mt.z - ms.z)
 *               R = Rz(c,s) = [[c,-s,0],[s,c,0],[0,0,1]] for f = 0 and Rz(c,s) diag(1,-1,1) = [[c,s,0],[s,-c,0],[0,0,1]]
 *               for f = 1 (a negation changes the sign bit only; u and ms under f = 1 are (ux, -uy) and (ms.x, -ms.y,
 *               ms.z)).  M = the row-major 4x4 [R | T], last row 0 0 0 1, laid out like vcp_icp_multistart's
 *   score       the landmarks are vcp_icp_vtklike's: every step-th source point, step = ns / max_landmarks when
 *               ns > max_landmarks (ns / step of them).  Each is moved by M as vcp_match moves a centroid (row by row,
 *               left to right, all four terms) and counts when SOME target has sqrt(dx*dx + dy*dy + dz*dz) <
 *               inlier_dist, dx = target.x - moved.x and so on: vcp_match's expression and operand order, strict
 *   per base    the hypothesis with the highest score wins, ties to the lowest (f, i, j) lexicographically:
 *               score [n_bases], pick [n_bases*3] = (f, i, j), M_all [n_bases*16]; n_hyp [n_bases] = the exact number of
 *               hypotheses of the base.  A base without a hypothesis that was scored: score -1, pick (0, -1, -1), a zero
 *               M, inliers 0
 *   inliers [n_bases]  the same count as the score taken over ALL ns source points under the base's winner; for
 *               all-finite input inliers[b] == vcp_match(source, target, M_b, inlier_dist).count_matched
 *   best        the base with the most inliers among those with score >= 0, ties to the higher score, then the lower b;
 *               M_best = its matrix.  No such base: VCP_OK, *best = -1, M_best = the identity
 * M_all, score, inliers, pick, n_hyp may each be NULL; M_best, best and bases are required.  VCP_ERR_ARG: a NULL required
 * pointer, n_bases < 1, max_landmarks < 1, len_tol NaN or < 0, inlier_dist NaN or <= 0 (len_tol = 0, len_tol = +inf and
 * inlier_dist = +inf are valid); VCP_ERR_EMPTY: ns < 2 or nt < 2; VCP_ERR_UNSUPPORTED: n_bases > 4096 (vcp_icp_gated's
 * pose limit: the winners can be fed to it) or nt > 65 536 (the pair enumeration is quadratic in nt by design);
 * VCP_ERR_TOO_LARGE: ns >= 2^31.  Nothing is written on an error.
 * There is no list of hypotheses and no cap on their number: they are scored as they are found.  Deterministic: only
 * integer comparisons and integer atomics decide anything, two calls give identical bits.  Timing phases: regp_grid
 * (bases and the target grid), regp_search, regp_final (csrc/register.hip). */
int vcp_register_pairs(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                       const int32_t* bases, int32_t n_bases, double len_tol, int mirror, int max_landmarks,
                       double inlier_dist, double M_best[16], int32_t* best, double* M_all, int32_t* score,
                       int32_t* inliers, int32_t* pick, int64_t* n_hyp);
/* Same with device pointers for source, target, bases and the five per-base arrays, on the context's stream; M_best
 * and best stay host pointers; returns when the result is in place. */
int vcp_register_pairs_dev(vcp_ctx* ctx, const double* d_source, int64_t ns, const double* d_target, int64_t nt,
                           const int32_t* d_bases, int32_t n_bases, double len_tol, int mirror, int max_landmarks,
                           double inlier_dist, double M_best[16], int32_t* best, double* d_M_all, int32_t* d_score,
                           int32_t* d_inliers, int32_t* d_pick, int64_t* d_n_hyp);

/* Self-test of the pose arithmetic of vcp_register_pairs, run on the HOST from the same source the device executes: the
 * base (a, b'), the targets t_i, t_j and the flip f give Lu_Lv = (Lu, Lv) and, when the hypothesis is not skipped, M.
 * Returns 1 (M written), 0 (skipped: nrm is not in (0, inf); M untouched) or VCP_ERR_ARG (a NULL pointer).  The length
 * test against len_tol is the caller's.  Needs no device and no context. */
int vcp_selftest_register_pose(const double a[3], const double b[3], const double ti[3], const double tj[3], int f,
                               double Lu_Lv[2], double M[16]);

/* -- scale-free registration by similarity pairs -------------------------------------------------------
 * vcp_register_pairs assumes that source and targets are in one unit.  The reference brings a scan to the truths' unit by
 * the ratio of the two bounding boxes (MainForm.showTruesAndCenters, FrmMain.cs:3030-3055), which is wrong for a scan that
 * sees part of the field and moves with one false cluster at the edge.  This call lets the pair carry the scale: a base
 * laid on an ordered pair of targets whose length is k times its own, scale_min <= k <= scale_max, is a planar similarity.
 * Everything not named here is vcp_register_pairs's, word for word: bases, flip, Lu, Lv, the landmarks, the score (strict
 * <), the per-base winner (highest score, ties to the lowest (f, i, j)), inliers over all ns, best, the limits, which
 * outputs may be NULL, "nothing written on an error".  binary64, every operation rounded on its own.
 *   hypothesis  k = Lv / Lu (one correctly rounded division).  (b, f, i, j) is a HYPOTHESIS iff 0 < Lu < inf,
 *               0 < Lv < inf and scale_min <= k && k <= scale_max.  The division is the test: no product form, no squared
 *               lengths.  Comparisons with NaN are false
 *   pose        dot, crs, nrm, c, s, the midpoints and the sign handling under f = 1 are vcp_register_pairs's; skipped
 *               (still counted in n_hyp) unless 0 < nrm < inf.  kc = k*c, ks = k*s.
 *               T = (mt.x - (kc*ms.x - ks*ms.y), mt.y - (ks*ms.x + kc*ms.y), mt.z - k*ms.z)
 *               R = [[kc,-ks,0],[ks,kc,0],[0,0,k]] for f = 0, [[kc,ks,0],[ks,-kc,0],[0,0,k]] for f = 1; M as before.
 *               Where k == 1.0 exactly, M is vcp_register_pairs's bit for bit (1.0 * x is x, the sign of a zero included)
 *   scale [n_bases]  (may be NULL) the winner's k; 0.0 for a base without a hypothesis that was scored
 * VCP_ERR_ARG: scale_min NaN or <= 0; scale_max NaN, +inf or < scale_min (scale_min == scale_max is valid); the other
 * errors are vcp_register_pairs's.  Timing phases: regs_grid, regs_search, regs_final (csrc/register.hip, DESIGN.md
 * section 18). */
int vcp_register_sim(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                     const int32_t* bases, int32_t n_bases, double scale_min, double scale_max, int mirror,
                     int max_landmarks, double inlier_dist, double M_best[16], int32_t* best, double* M_all, int32_t* score,
                     int32_t* inliers, int32_t* pick, int64_t* n_hyp, double* scale);
/* Same with device pointers for source, target, bases and the six per-base arrays, on the context's stream; M_best and
 * best stay host pointers; returns when the result is in place. */
int vcp_register_sim_dev(vcp_ctx* ctx, const double* d_source, int64_t ns, const double* d_target, int64_t nt,
                         const int32_t* d_bases, int32_t n_bases, double scale_min, double scale_max, int mirror,
                         int max_landmarks, double inlier_dist, double M_best[16], int32_t* best, double* d_M_all,
                         int32_t* d_score, int32_t* d_inliers, int32_t* d_pick, int64_t* d_n_hyp, double* d_scale);

/* Self-test of the pose arithmetic of vcp_register_sim, run on the HOST from the source the device executes:
 * Lu_Lv_k = (Lu, Lv, k = Lv / Lu) and, when the hypothesis is not skipped, M.  Returns 1 (M written), 0 (skipped: nrm is
 * not in (0, inf); M untouched) or VCP_ERR_ARG (a NULL pointer).  The test of k against the range is the caller's.  Needs
 * no device and no context. */
int vcp_selftest_register_sim_pose(const double a[3], const double b[3], const double ti[3], const double tj[3], int f,
                                   double Lu_Lv_k[3], double M[16]);

/* -- minimal bounding circles ---------------------------------------------
 * Replaces Tools.getCircles (BC/Tools.cs:394-409) / Geometry.FindMinimalBoundingCircle
 * (BC/Geometry.cs:247-319; gift-wrap hull :122-208, circle through 2 or 3 hull points :260-312): for
 * every cluster 1..K with more than 3 points the smallest enclosing circle of its (x,y).
 * xy [n*2] = (X,Y) for the 3-D view or (motor_x,motor_y) for the 2-D one; labels [n]; order [m] = the
 * list order the C# iterates (clusForMerge; NULL = 0..n-1, then m must equal n): "first in the list"
 * decides every tie.  centers [K*2], radius [K], valid [K] (0 = cluster skipped), hull_n [K] may be NULL.
 * The C# arithmetic (binary64, no FMA contraction), bit for bit, wherever its circle encloses the cluster.  Two rules
 * of this library's own stand behind it, for the two cases in which it does not; both are exact comparisons of the
 * expression d(p) = (cx-p.x)*(cx-p.x) + (cy-p.y)*(cy-p.y), so host and device agree to the bit.  S is the hull, then
 * the members rule 2 added, in that order (the search's loop order over S breaks its ties):
 *   1. covering:  if no pair and no triple of S encloses S (points on a common circle up to rounding: every candidate
 *      loses another point by an ulp, and the C# returns radius 0 around points[0]), the search over the pairs, then
 *      the triples runs again and a candidate counts with max over S of d(p) from its centre instead of its own
 *      radius^2; the smallest wins, the first on ties, and radius^2 is that maximum.
 *   2. insertion: the gift wrap can close early on a cluster that is collinear up to rounding (the pseudo-angle to the
 *      next point on the line falls an ulp below the sweep), and the hull then lacks true extreme points.  While a
 *      member has d(p) strictly greater than every point of S (a NaN d(p) of a point of S: nothing is greater; of a
 *      member: it is no candidate), the member with the largest d(p), the first in list order on ties, is appended to
 *      S and the search runs again, rule 1 included.  More than 2048 points in S: VCP_ERR_TOO_LARGE.
 * hull_n counts the wrap's hull: it can be incomplete for such clusters; the circle is not affected by that. */
int vcp_mcc(vcp_ctx* ctx, const double* xy, const int32_t* labels, const int64_t* order, int64_t m,
            int64_t n, int32_t K, double* centers, double* radius, uint8_t* valid, int32_t* hull_n);

/* -- cluster shapes and the radius / aspect filter ------------------------------------------------
 * The reference rejects clusters "based on the circumscribed circle and the circumscribed rectangle" (its README):
 * MainForm.FilterClustersByRadius (FrmMain.cs:1905-1920: radius > r fills filterID) and removePointByRadius
 * (:3743-3746 -> Tools.removeFilterPointFromClustering, BC/Tools.cs:70-74, a stable RemoveAll).  One pass per cluster
 * gives the convex hull, the minimal bounding circle and the minimum-area bounding rectangle.
 *
 * Inputs and the circle outputs (centers, radius, valid, hull_n) are vcp_mcc's, bit for bit.
 *
 * Hull.  The hull of cluster k is the array hull[0..h) vcp_mcc builds (Geometry.MakeConvexHull, BC/Geometry.cs:122-208:
 * lowest y then lowest x, gift wrapping on the pseudo-angle, first in list order on ties; `order` decides list order).
 * It is returned as indices into the caller's point array: hull_off [K+1] = prefix sums of the hull sizes
 * (hull_off[0] = 0; a cluster with valid != 1 contributes 0), hull_idx [hull_off[K]] (the caller provides room for m
 * entries).  Among points with equal coordinates the index is the one the C# picks: the first in list order that is
 * still in the list.  hull_n, hull_off and hull_idx describe the wrap's hull: for a cluster collinear up to rounding
 * it can lack extreme points (vcp_mcc, rule 2); the circle and the rectangle are not affected by that.
 *
 * Rectangle.  All arithmetic binary64, every operation rounded on its own, sqrt and / correctly rounded.  For hull
 * edge i, a = hull[i], b = hull[(i+1) % h]:
 *     dx = b.x - a.x;  dy = b.y - a.y;  L2 = dx*dx + dy*dy              edge skipped unless 0 < L2 < +inf
 *     for every hull point p:  rx = p.x - a.x;  ry = p.y - a.y
 *                              u = rx*dx + ry*dy;   v = ry*dx - rx*dy
 *     U = max u - min u;  V = max v - min v;  area_i = (U * V) / L2
 * Minima and maxima are exact; one that is zero counts as +0; a NaN among the u, v makes the edge no candidate, and so
 * does an area that is not < +inf.  The rectangle of the cluster is that of the candidate with the smallest area_i,
 * the lowest i on ties (that a minimum-area enclosing rectangle has a side on a hull edge: Freeman & Shapira 1975).
 * For a cluster on which vcp_mcc's rule 2 appended a member, "every hull point p" reads "every member p of the cluster
 * other than (NaN, NaN)": the edges stay the wrap's, the extents span the members, so the rectangle contains them.
 *   rect_valid [K]   1 when valid == 1 and some edge is a candidate (for finite input that does not overflow:
 *                    valid == 1 && hull_n >= 2), else 0; then rect_len = 0, rect_edge = -1 and the four corners are
 *                    hull[0] (valid == 1) or (0, 0) (valid == 0: a cluster of <= 3 points has no hull)
 *   rect_edge [K]    the chosen i
 *   rect_len [K*2]   (U / sqrt(L2), V / sqrt(L2)): the side along the hull edge first
 *   rect_xy [K*8]    the corners (min u, min v), (max u, min v), (max u, max v), (min u, max v) as
 *                    x = a.x + (u*dx - v*dy) / L2,  y = a.y + (u*dy + v*dx) / L2
 * Any of the four rect_* may be NULL; hull_off and hull_idx: both or neither; hull_n may be NULL.  With all six NULL
 * the call is vcp_mcc.  This is the rectangle by definition, not a port: BC/Polygon.cs (FindSmallestBoundingRectangle)
 * has no caller in the reference and is not transcribed.
 * Errors and limits are vcp_mcc's: a label outside 0..K VCP_ERR_INDEX, a hull beyond 2048 points VCP_ERR_TOO_LARGE, a
 * cluster without a finite point VCP_ERR_EMPTY; K == 0 does nothing.  Deterministic.  Timing phases: shapes_group
 * (members by cluster), shapes_fit (hull + circle + rectangle, one kernel), shapes_hull (offsets and export). */
int vcp_cluster_shapes(vcp_ctx* ctx, const double* xy, const int32_t* labels, const int64_t* order, int64_t m,
                       int64_t n, int32_t K, double* centers, double* radius, uint8_t* valid, int32_t* hull_n,
                       double* rect_xy, double* rect_len, int32_t* rect_edge, uint8_t* rect_valid,
                       int32_t* hull_off, int32_t* hull_idx);
/* Same with device pointers, on the context's stream; returns when the result is in place (K bytes are read back for
 * the error check). */
int vcp_cluster_shapes_dev(vcp_ctx* ctx, const double* d_xy, const int32_t* d_labels, const int64_t* d_order,
                           int64_t m, int64_t n, int32_t K, double* d_centers, double* d_radius, uint8_t* d_valid,
                           int32_t* d_hull_n, double* d_rect_xy, double* d_rect_len, int32_t* d_rect_edge,
                           uint8_t* d_rect_valid, int32_t* d_hull_off, int32_t* d_hull_idx);

/* The filter.  Plain comparisons, so a NaN or +inf threshold switches its criterion off, as `radius > r` does in the C#:
 *     filtered[k] = valid[k] == 1 && ( radius[k] > max_radius
 *                                   || (rect_valid[k] == 1 && max(len0, len1) > max_aspect * min(len0, len1)) )
 *     keep[i]     = !(1 <= labels[i] <= K && filtered[labels[i] - 1])         label 0 (noise) is always kept
 *     kept_idx    = the indices i with keep[i], ascending (RemoveAll is stable); *n_kept of them
 * No division: a cluster on a line (V == 0) is filtered by any finite max_aspect, a single repeated point by none.
 * labels [n]; radius, valid [K]; rect_len [K*2] and rect_valid [K] may be NULL together (no aspect criterion);
 * filtered [K] (the reference's filterID as flags; *n_filtered of them set); keep [n] and kept_idx [n] may be NULL,
 * n_filtered and n_kept too.  Cluster ids are not renumbered (the C# does not either).  A label outside 0..K is
 * VCP_ERR_INDEX.  Timing phase: filter. */
int vcp_cluster_filter(vcp_ctx* ctx, const int32_t* labels, int64_t n, int32_t K, const double* radius,
                       const uint8_t* valid, const double* rect_len, const uint8_t* rect_valid, double max_radius,
                       double max_aspect, uint8_t* filtered, uint8_t* keep, int32_t* kept_idx, int32_t* n_filtered,
                       int64_t* n_kept);
/* Same with device pointers; the two counts stay host pointers (16 bytes read back). */
int vcp_cluster_filter_dev(vcp_ctx* ctx, const int32_t* d_labels, int64_t n, int32_t K, const double* d_radius,
                           const uint8_t* d_valid, const double* d_rect_len, const uint8_t* d_rect_valid,
                           double max_radius, double max_aspect, uint8_t* d_filtered, uint8_t* d_keep,
                           int32_t* d_kept_idx, int32_t* n_filtered, int64_t* n_kept);

/* -- matching ------------------------------------------------------------------------------
 * Replaces MainForm.calMatchedCoords (FrmMain.cs:3572-3587) + RecorrectMatchingPtsByDistance
 * (:3588-3618, getDisP :829-835): matched = M * (c,1); nearest truth by Euclidean distance
 * (strict <, lowest index on ties); is_matched iff distance < max_dist.  K == 0 does nothing; K > 0 && T == 0:
 * VCP_ERR_EMPTY (the C# reads truePointCloud.GetPoint(0), :3598). */
int vcp_match(vcp_ctx* ctx, const double* centers, int32_t K, const double* truths, int32_t T,
              const double M[16], double max_dist, double* matched_xyz, uint8_t* is_matched,
              int32_t* nearest, double* nearest_dist, int32_t* count_matched);

/* -- one-to-one matching ----------------------------------------------------------------------------
 * vcp_match lets two centroids take the same truth (the C# does: nothing in FrmMain.cs:3588-3618 stops it), so matchedID
 * and the exported (centroid, truth) list (:1696-1698) can hold one truth twice.  vcp_match_unique returns a pairing: no
 * centroid and no truth appears in two pairs.  It has no counterpart in the reference; vcp_match is unchanged.
 *   transform   m_j = M * (c_j, 1), row by row, left to right, no contraction: vcp_match's
 *   distance    d(j,i) = sqrt(dx*dx + dy*dy + dz*dz), dx = truths[3i] - m_j[0] and so on: binary64, correctly rounded
 *               sqrt, vcp_match's expression and operand order
 *   candidates  E = { (j,i) : d(j,i) < max_dist }, a strict comparison.  A NaN distance is never a candidate and a +inf
 *               distance neither, not even with max_dist = +inf: a centroid or truth with a non-finite coordinate pairs
 *               with nobody
 *   matching    walk E in ascending order of the key (d, j, i) -- equal distances go to the lower centroid index, then
 *               to the lower truth index -- and accept a pair when neither end is taken yet.  This sequential greedy
 *               walk is the specification (tests/match_unique_ref.py restates it in numpy; results are compared bit
 *               for bit).  The device computes it by rounds of locally dominant pairs: in a round every pair that is
 *               the minimum-key candidate of both of its ends, among the points still free, is accepted at once, until
 *               a round accepts nothing.  The key order is strict and total, so both give the same pairing (DESIGN.md
 *               section 15)
 *   truth_of [K]      index of the paired truth, -1 when none
 *   center_of [T]     the inverse, -1 when none: the unmatched-truth list the reference displays
 *   pair_dist [K]     may be NULL: d of the pair, +inf when unpaired
 *   matched_xyz [K*3] may be NULL: bit-identical to vcp_match's
 *   *count_pairs      may be NULL: the number of pairs
 *   *rounds           may be NULL: the number of rounds that accepted a pair; informative, <= min(K, T)
 * Every truth vcp_match gives to some matched centroid is paired here; where vcp_match's nearest is injective on its
 * matched centroids the two calls agree (truth_of[j] = nearest[j] where matched, -1 elsewhere, equal counts).
 * K == 0 does nothing (center_of is filled with -1 when T > 0); K > 0 && T == 0: VCP_ERR_EMPTY; NULL M, truth_of or
 * center_of: VCP_ERR_ARG.  max_dist NaN or <= 0 is no error: E is empty, zero pairs, VCP_OK (the C#'s plain `<`).
 * Candidates come from a 3-D grid over the truths with a cell edge of max_dist or more (at most 2^22 cells), built per
 * call in its own workspace.  max_dist = +inf, or a box that needs a cell edge beyond its extent, is one cell, that is
 * all K * T pairs per round: slow and correct.  The worst case in rounds is a chain (each pair becomes dominant only when
 * the one before it is gone): min(K, T) rounds of three small kernels each.
 * Deterministic: two calls on the same input give identical bits, and the result does not depend on scheduling (only
 * integer min-atomics decide it).  Timing phases: matchu_grid, matchu_rounds (csrc/match_unique.hip). */
int vcp_match_unique(vcp_ctx* ctx, const double* centers, int32_t K, const double* truths, int32_t T,
                     const double M[16], double max_dist, double* matched_xyz, int32_t* truth_of, int32_t* center_of,
                     double* pair_dist, int32_t* count_pairs, int32_t* rounds);
/* Same with device pointers (d_matched_xyz, d_pair_dist may be NULL), on the context's stream; M, count_pairs and rounds
 * stay host pointers; returns when the result is in place. */
int vcp_match_unique_dev(vcp_ctx* ctx, const double* d_centers, int32_t K, const double* d_truths, int32_t T,
                         const double M[16], double max_dist, double* d_matched_xyz, int32_t* d_truth_of,
                         int32_t* d_center_of, double* d_pair_dist, int32_t* count_pairs, int32_t* rounds);

/* -- import conversion + duplicate removal ------------------------------------
 * Replaces the per-row work of MainForm.AddFolder for scan points (FrmMain.cs:1011-1090, typpe 1 / 2):
 * rows [n*3] = (motor_x, motor_y, Distance) as parsed from the tab-separated text (BC/FileMap.cs:16-33);
 * rows with Distance == 0 or > 1000 are filtered (:1011); X,Y,Z by the spherical conversion of :1025-1062 with
 * the zero angles x_angle, y_angle and the axis choices xdir, ydir (1 up, 2 right, 3 down, 4 left); with
 * dedupe != 0 a row whose (tmpx,tmpy,tmpz) equals that of an earlier kept row is a duplicate (:1063-1068; the
 * C#'s O(n^2) FindAll becomes a device hash table).  xyz [n*3] and state [n] (0 filtered, 1 kept, 2 duplicate)
 * are written for every row in input order.  dedupe needs the ImportPts defaults xdir = 2, ydir = 1. */
int vcp_import_convert(vcp_ctx* ctx, const double* rows, int64_t n, double x_angle, double y_angle, int xdir,
                       int ydir, int dedupe, double* xyz, uint8_t* state, int64_t* kept, int64_t* duplicates);

/* -- resident import: filter, dedupe with counts, compact ---------------------------------------------
 * vcp_import_convert writes xyz and state for EVERY row and leaves the selection to the host.  This call keeps the scan on
 * the device: it filters, finds the duplicate classes with their sizes, and writes the kept rows densely, in input order,
 * in the layout vcp_dbscan_dev / vcp_gdbscan_dev / vcp_centroids_dev take.  With a group number per row it is also
 * AddFolder's fixed-point import, typpe 3 / 4 (FrmMain.cs:1069-1085), whose duplicates are searched per file and whose
 * kept row's ptsCount goes up (:1074, :1081): the producer of vcp_centroids_weighted's group / pts_count.
 *   row        row i is rows[3i..3i+2] = (mx, my, D).  It is filtered iff D == 0 || D > 1000, the plain comparisons of
 *              FrmMain.cs:1011: a NaN D is not filtered.  (tx, ty, tz) = (tmpx, tmpy, tmpz) and (X, Y, Z) are
 *              vcp_import_convert's for x_angle, y_angle, xdir, ydir: bit for bit what it writes for that row on the same
 *              device (the same kernel).  g_i = group[i], or 0 when group == NULL; any int32 is a valid group
 *   classes    dedupe == 0: every unfiltered row is a class of its own.  dedupe != 0: unfiltered rows i, j are in one
 *              class iff g_i == g_j && tx_i == tx_j && ty_i == ty_j && tz_i == tz_j under the C#'s `==`: -0 equals +0, and
 *              a triple holding a NaN equals nothing, so its row is a class of its own.  The class keeps its smallest row
 *              index, the first occurrence -- what the sequential FindAll / FindIndex keep.  group == NULL is typpe 1 (the
 *              whole list), group = the file number is typpe 3 / 4
 *   outputs    the m kept rows in ascending order of their input index (stable); the caller provides room for n entries;
 *              each array may be NULL
 *     src [m]        the input index of the kept row
 *     motor [m*2]    its (mx, my)
 *     dist [m]       its D
 *     xyz [m*3]      its own (X, Y, Z): the first occurrence's bits, -0 included
 *     count [m]      the size of its class (Point3D.ptsCount; 1 without dedupe)
 *     group_out [m]  its g
 *     row_to [n]     for every input row the compact position of its class's kept row, -1 for a filtered row: the labels
 *                    of the raw rows are labels[row_to]
 *     *m             required; *duplicates (may be NULL) = unfiltered rows - m
 * With group == NULL, src is exactly the indices where vcp_import_convert(..., dedupe) has state == 1, xyz equals its
 * xyz[src] bit for bit and duplicates equals its count; sum(count) == the number of unfiltered rows.
 * Nothing is written on an error.  VCP_ERR_ARG: NULL ctx, NULL m, NULL rows with n > 0, n < 0, a direction outside 1..4;
 * VCP_ERR_UNSUPPORTED: dedupe with directions other than xdir 2 / ydir 1, for the reason vcp_import_convert gives;
 * VCP_ERR_TOO_LARGE: n >= 0x7FFFFFF0.  n == 0: *m = 0, VCP_OK.  The outputs must not overlap the inputs.
 * The result is a function of the input alone: only integer atomics decide anything (a minimum for the kept index, a sum
 * for the count); two calls give identical bits, and so does a call after any other call on the context.
 * Timing phases: impc_convert, impc_dedupe, impc_compact (csrc/import.hip). */
int vcp_import_compact(vcp_ctx* ctx, const double* rows, int64_t n, const int32_t* group, double x_angle, double y_angle,
                       int xdir, int ydir, int dedupe, double* motor, double* xyz, double* dist, int32_t* src,
                       int32_t* count, int32_t* group_out, int32_t* row_to, int64_t* m, int64_t* duplicates);
/* Same with device pointers for rows, group and the seven arrays, on the context's stream under the vcp_set_stream
 * contract; m and duplicates stay host pointers.  One synchronisation, for the two counts; returns when the result is in
 * place. */
int vcp_import_compact_dev(vcp_ctx* ctx, const double* d_rows, int64_t n, const int32_t* d_group, double x_angle,
                           double y_angle, int xdir, int ydir, int dedupe, double* d_motor, double* d_xyz, double* d_dist,
                           int32_t* d_src, int32_t* d_count, int32_t* d_group_out, int32_t* d_row_to, int64_t* m,
                           int64_t* duplicates);

/* -- truth-guided assignment -------------------------------------------------
 * Replaces the query of MainForm.refreshClusList (FrmMain.cs:3437-3467): per raw point (motor_x, motor_y)
 * the nearest truth (tmp_X, tmp_Y) with Euclidean distance < radius; among equal distances the LAST truth
 * in list order wins (OrderByDescending(DISTANCE).Reverse()); ids[i] = that truth's clusterId, 0 = none;
 * *outliers = number of points with id 0 ("yedian"). */
int vcp_assign_truths(vcp_ctx* ctx, const double* motor, int64_t n, const double* truths_xy,
                      const int32_t* truth_ids, int32_t T, double radius, int32_t* ids, int64_t* outliers);

/* -- k-distance ---------------------------------------------------------------------------------
 * The k-distance graph of Ester et al. (1996) for choosing DBSCAN's eps (the reference types eps by hand:
 * Clustering.Designer.cs:86,96, ClusterByMatlab.Designer.cs:86,96).  Exact k nearest neighbours of every point:
 *   d(i,j)     the binary64 expression vcp_dbscan tests: VCP_L1_2D |dx| + |dy|, VCP_L2_2D sqrt(dx*dx + dy*dy),
 *              VCP_L2_3D sqrt(dx*dx + dy*dy + dz*dz) (sums left to right, no FMA contraction, correctly rounded
 *              sqrt); VCP_SIGNED_SUM_2D = VCP_ERR_ARG
 *   kdist[i]   the k-th smallest value of the multiset { d(i,j) : j = 0..n-1 } -- j = i INCLUDED, like the core
 *              count of DBImproved.isKeyPoint -- so that for every finite eps >= 0
 *                vcp_dbscan(..., eps, min_pts = k, in_classed = NULL).is_core[i] == (kdist[i] <= eps)
 *              bit for bit
 *   knn [n*k]  may be NULL: row i = the k indices j with the smallest (d(i,j), j) pairs, ascending (a lower index
 *              wins a tie); the last one's value is kdist[i]
 * A point with a NaN / infinite coordinate has no neighbour, not even itself: kdist NaN, knn row all -1, and it is
 * nobody's candidate.  A finite point with fewer than k finite points in the cloud: kdist +inf, the missing slots -1.
 * coords [n*dim] point-major, dim 2 or 3 (the 2-D metrics read x, y; VCP_L2_3D needs dim 3).  Limits: 1 <= k <= 64
 * (k < 1: VCP_ERR_ARG, k > 64: VCP_ERR_UNSUPPORTED), n < 2^31 (int32 indices; VCP_ERR_TOO_LARGE beyond); a cloud whose
 * coordinate differences overflow binary64 is VCP_ERR_UNSUPPORTED, as in vcp_dbscan.  n = 0 does nothing.
 * Deterministic: two calls on the same input give identical bits.  Timing phases: kdist_bounds, kdist_order,
 * kdist_search, kdist_heavy (csrc/kdist.hip). */
int vcp_kdist(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, int k, double* kdist,
              int32_t* knn);
/* Same with device pointers (d_knn may be NULL), on the context's stream; returns when the result is in place. */
int vcp_kdist_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, int k, double* d_kdist,
                  int32_t* d_knn);

/* -- eps tree -------------------------------------------------------------------------------------
 * The knee of the k-distance graph knows nothing about the clusters the caller wants; a caller who knows the number of
 * targets wants an eps at which vcp_dbscan finds about that many clusters.  For a fixed min_pts = k this call returns
 * what vcp_dbscan decides at EVERY eps <= eps_max at once.  It has no counterpart in the reference.  All values are
 * selections among binary64 numbers vcp_kdist defines: no new rounding.
 *   d, kdist    d(i,j) and kdist[i] are vcp_kdist's (VCP_L1_2D, VCP_L2_2D, VCP_L2_3D; j = i included); a point with a
 *               non-finite coordinate has kdist NaN and takes part in nothing
 *   kdist       kdist_given == 0: kdist [n] is an output and may be NULL; it is computed by the code of vcp_kdist_dev.
 *               kdist_given != 0: kdist is required and read as given; the caller vouches that it is vcp_kdist's for the
 *               same coords, metric and k (suggest_eps has computed it already).  A call with kdist_given != 0 on an
 *               earlier call's output gives identical bits
 *   vertices    P = { i : kdist[i] <= eps_max }: the points that are core at some eps <= eps_max
 *   edges       E = { (i,j) : i < j, both in P, d(i,j) <= eps_max }, w(i,j) = max(kdist[i], kdist[j], d(i,j)) (a
 *               selection; the mutual-reachability distance): i and j are linked core points at eps iff w(i,j) <= eps.
 *               Edges are ordered by the key (w, i, j), lexicographic: a strict total order
 *   forest      the minimum spanning forest of (P, E) under that order is unique and equals the edges a Kruskal walk over
 *               E in ascending key order accepts.  That sequential walk is the specification (tests/eps_tree_ref.py
 *               restates it in numpy; results are compared bit for bit).  *n_merge = the number of accepted edges;
 *               merge_w, merge_a, merge_b hold them in ascending key order, a < b indices into the caller's array; the
 *               caller provides room for max(n - 1, 0) entries.  merge_a and merge_b: both or neither; merge_w and
 *               n_merge are required.  The device computes the forest by Boruvka rounds
 *   reach [n]   may be NULL: reach[i] = min over j in P (j = i included) with d(i,j) <= eps_max of max(kdist[j], d(i,j));
 *               +inf when there is no such j, NaN for a non-finite point
 * For all-finite input and every finite eps with 0 <= eps <= eps_max, r = vcp_dbscan(coords, eps, min_pts = k,
 * cf_in = 0, in_classed = NULL) satisfies
 *     sum(r.is_core)      == #{ kdist <= eps }
 *     r.cf_out            == #{ kdist <= eps } - #{ merge_w <= eps }
 *     #{ r.labels != 0 }  == #{ reach <= eps }
 *     two core points of r share a label iff the forest edges with w <= eps connect them.
 *   *rounds     may be NULL: the number of device rounds that accepted an edge; informative, <= floor(log2 |P|) and 0
 *               when |P| < 2 (a tree that accepts an edge in round r has at least 2^(r-1) vertices, and so has the tree
 *               it joins)
 * Nothing is written on an error.  VCP_ERR_ARG: a NULL required pointer, merge_a without merge_b or the reverse,
 * kdist_given with NULL kdist, dim not 2 or 3, VCP_L2_3D with dim 2, VCP_SIGNED_SUM_2D, k < 1, eps_max NaN, <= 0 or +inf;
 * VCP_ERR_UNSUPPORTED: k > 64, an extent that overflows, as in vcp_kdist; VCP_ERR_TOO_LARGE: n >= 2^31.  n == 0:
 * *n_merge = 0, VCP_OK.
 * Candidates come from a uniform grid over the finite points with a cell edge of eps_max or more (at most 2^22 cells),
 * built per call in its own workspace; an eps_max beyond the cloud's extent is one cell, that is all pairs per round: slow
 * and correct.  Deterministic: only integer min-atomics decide anything, two calls give identical bits.  Timing phases:
 * epst_kdist (absent when given), epst_grid, epst_rounds, epst_reach, epst_sort (csrc/eps_tree.hip). */
int vcp_eps_tree(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, int k, double eps_max,
                 int kdist_given, double* kdist, double* reach, int64_t* n_merge, double* merge_w, int32_t* merge_a,
                 int32_t* merge_b, int32_t* rounds);
/* Same with device pointers for coords, kdist, reach, merge_w, merge_a, merge_b, on the context's stream; n_merge and
 * rounds stay host pointers; returns when the result is in place. */
int vcp_eps_tree_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, int k, double eps_max,
                     int kdist_given, double* d_kdist, double* d_reach, int64_t* n_merge, double* d_merge_w,
                     int32_t* d_merge_a, int32_t* d_merge_b, int32_t* rounds);

/* -- generalised DBSCAN: point weights and a range gate -----------------------------------------------
 * vcp_dbscan decides what DBImproved decides: every row counts once, and two rows are neighbours whenever their
 * coordinates are within eps.  This call generalises both (sample_weight of scikit-learn's DBSCAN, MinWeight of GDBSCAN,
 * Sander et al. 1998; a neighbourhood predicate with a second test) and is otherwise the same algorithm.  It has no
 * counterpart in the reference, whose answers are to drop duplicates (FrmMain.cs:1063-1068) and to cut one global band
 * of Distance (Tools.FilterByDistance_ScanPoint, Tools.cs:416-431).
 *   d(i,j)     vcp_kdist's binary64 expression for VCP_L1_2D, VCP_L2_2D, VCP_L2_3D (sums left to right, no FMA
 *              contraction, correctly rounded sqrt); VCP_SIGNED_SUM_2D = VCP_ERR_ARG
 *   N(i)       { j : d(i,j) <= eps and (aux == NULL or fabs(aux[i] - aux[j]) <= gate) }, both tests in binary64, j = i
 *              included.  A row with a non-finite coordinate has an empty N and is in nobody's N; so has a row with a
 *              non-finite aux[i] when aux is given.  eps NaN or < 0 makes every N empty (by the expression; not an error,
 *              as in vcp_dbscan)
 *   W(i)       the sum over j in N(i) of w[j], in int64; w[j] = weights[j], or 1 when weights == NULL.  Weights are
 *              >= 0; a row of weight 0 adds nothing to any sum and is labelled like any other row
 *   core[i]    <=> W(i) >= min_weight.  So min_weight <= 0 makes every row core, and a non-finite row then is a cluster
 *              of its own, as in the literal C#
 *   clusters   the connected components of the core points under j in N(i) (symmetric), numbered cf_in + 1,
 *              cf_in + 2, ... by increasing smallest member index.  A non-core point with a core point in its N takes
 *              the LARGEST such id (BC/DBImproved.cs:87); every other point gets 0.  *cf_out = cf_in + the number of
 *              clusters
 * With weights == NULL and aux == NULL this is vcp_dbscan(in_classed = NULL) with min_pts = min_weight.  With integer
 * weights >= 1 it is vcp_dbscan on the cloud in which row j stands w[j] times, restricted to the first copies --
 * wherever the copies of a row are neighbours of each other, that is for min_weight >= 1, or for eps >= 0 and rows
 * without a non-finite coordinate.  (A row with an empty N is core only for min_weight <= 0; here it is one cluster
 * whatever its weight, there every copy is a cluster of its own: the labels of the first copies agree, cf_out does not.)
 * coords [n*dim] point-major, dim 2 or 3 (the 2-D metrics read x, y; VCP_L2_3D needs dim 3); aux [n] or NULL;
 * weights [n] or NULL; labels [n] out; is_core [n] and wsum [n] out, either may be NULL.  wsum, when given, is W(i)
 * exactly for every row (0 for a row with an empty N); when it is NULL the count stops at min_weight.
 * The result is a function of the input alone: two calls give identical bits, and so does a call after any other call
 * on the same context (the workspace is sized and cleared per call; only integer atomics decide anything).
 * Nothing is written on an error.  VCP_ERR_ARG: NULL ctx, NULL cf_out, NULL coords or labels with n > 0, n < 0, dim not
 * 2 or 3, VCP_L2_3D with dim 2, VCP_SIGNED_SUM_2D, aux given and gate NaN or < 0 (+inf is allowed), any weight < 0
 * (found on the device before any output is touched); VCP_ERR_TOO_LARGE: n >= 2^31; VCP_ERR_UNSUPPORTED: an extent
 * that overflows binary64, as in vcp_kdist.  n == 0: *cf_out = cf_in, VCP_OK.
 * Candidates come from a uniform grid over the finite rows on the coordinates only (aux is a filter, not an axis) with
 * a cell edge of eps or more (at most 2^22 cells), built per call in its own workspace; an eps of 0 or beyond the
 * cloud's extent is one cell, that is all pairs: slow and correct.  Timing phases: gdb_bounds, gdb_grid, gdb_count,
 * gdb_union, gdb_label (csrc/gdbscan.hip). */
int vcp_gdbscan(vcp_ctx* ctx, const double* coords, int64_t n, int dim, int metric, double eps, const double* aux,
                double gate, const int32_t* weights, int64_t min_weight, int32_t cf_in, int32_t* labels,
                uint8_t* is_core, int64_t* wsum, int32_t* cf_out);
/* Same with device pointers for coords, aux, weights, labels, is_core, wsum, on the context's stream; cf_out stays a
 * host pointer; returns when the result is in place. */
int vcp_gdbscan_dev(vcp_ctx* ctx, const double* d_coords, int64_t n, int dim, int metric, double eps,
                    const double* d_aux, double gate, const int32_t* d_weights, int64_t min_weight, int32_t cf_in,
                    int32_t* d_labels, uint8_t* d_is_core, int64_t* d_wsum, int32_t* cf_out);

/* -- per-cluster quantiles and MAD outlier rejection -----------------------------------------------------
 * Every other per-cluster number of this library is a mean (vcp_centroids, vcp_centroids_weighted) or a hull quantity
 * (vcp_cluster_shapes).  These calls give order statistics per cluster or group: the reference has Tools.GetGroupingManOrMin
 * (BC/Tools.cs:468-497: the min / max of Distance over all files, which seeds the dialog of SureDistanceFilter.cs:26-61) and
 * one hand-typed band of Distance for every file (Tools.FilterByDistance_FixedPoint, BC/Tools.cs:438-461, confirmed by
 * cleanDataByDistance2 :254-263) before getFixedPtsCentroid; one band cannot serve targets at different ranges.  All
 * outputs are selections among the caller's binary64 values, plus one rounded subtraction for the deviation.
 *   v_i        the value of row i is values[i * stride], stride >= 1 in doubles: a column of xyz is read in place.
 *              group[i] in 0..K; 0 = in no group, the convention of vcp_centroids_weighted; group k holds the rows with
 *              group[i] == k, c_k of them.  A label outside 0..K is VCP_ERR_INDEX, as in vcp_mcc
 *   order      with u the bit pattern of v: key(v) = 0xFFFFFFFFFFFFFFFF for any NaN, else u ^ 0x8000000000000000 when the
 *              sign bit is clear and ~u when it is set.  The unsigned order of the keys is the numeric order, with -0
 *              before +0 and NaN last.  Ties between equal keys need no rule: the output is the value
 *   rank       for a group of c >= 1 rows and q in [0, 1]: rank = (int64_t)floor(q * (double)(c - 1)), one multiplication
 *              in binary64; q = 0 is the minimum, q = 1 the maximum (GetGroupingManOrMin per list), q = 0.5 the LOWER median
 *   out        out[k * nq + j] = the value whose key has rank(q[j], c) (0-based, ascending) among the keys of group k + 1;
 *              a NaN is returned as 0x7FF8000000000000.  An empty group gives that NaN for every j and count 0, as
 *              vcp_centroids' empty clusters do.  counts [K] may be NULL
 *   MAD        med_k = the q = 0.5 selection of group k; dev_i = fabs(v_i - med_k), one subtraction in binary64 (no FMA);
 *              mad_k = the q = 0.5 selection of the group's dev; band = c_mad * mad_k; thr_k = band > floor ? band : floor,
 *              so a NaN band gives floor (an empty group: med and mad NaN, thr = floor, kept 0);
 *              reject[i] = group[i] >= 1 && !(dev_i <= thr_k): a NaN value is rejected, and floor = +inf rejects only
 *              those; reject is 0 for the rows of group 0.  kept[k] = the rows of group k + 1 that are not rejected,
 *              *n_rejected = the rejected rows in all.  All of med, mad, thr [K], reject [n], kept [K] and n_rejected are
 *              required
 * VCP_ERR_ARG: NULL ctx, a NULL required pointer (values or group with n > 0, q, out / med / mad / thr / kept with K > 0,
 * reject with n > 0, n_rejected), n < 0, K < 0, stride < 1, nq < 1, a q that is NaN or outside [0, 1], c_mad or floor NaN
 * or < 0; VCP_ERR_UNSUPPORTED: nq > VCP_CQ_NQ_MAX; VCP_ERR_TOO_LARGE: n >= 2^31; VCP_ERR_INDEX: a label outside 0..K, found
 * on the device before any output is touched.  Nothing is written on an error.  n == 0 or K == 0: nothing to select; the
 * outputs for K > 0 are the empty-group values (reject all 0 for K == 0), VCP_OK.
 * The rows are grouped by a stable sort on the label (as vcp_centroids does), the keys gathered in that order, and every
 * group is selected from by the class of its size: up to VCP_CQ_WAVE_MAX rows one wave ranks the keys by counting; up to
 * VCP_CQ_WG_MAX rows one workgroup holds the keys in LDS and runs an 8-bit radix select, most significant digit first;
 * larger groups share one histogram launch and one pick launch per digit.  The answer does not depend on the class, and all
 * nq ranks of a call share the grouping and the gather.  The result is a function of the input alone: only integer
 * comparisons and integer atomics decide which value is returned; two calls give identical bits, and so does a call after
 * any other call on the context.  Timing phases: cq_group, cq_select, and cq_flag for the MAD form
 * (csrc/cluster_quant.hip). */
#define VCP_CQ_WAVE_MAX 64
#define VCP_CQ_WG_MAX 4096
#define VCP_CQ_NQ_MAX 16
int vcp_cluster_quantiles(vcp_ctx* ctx, const double* values, int64_t stride, const int32_t* group, int64_t n, int32_t K,
                          const double* q, int32_t nq, double* out, int64_t* counts);
/* Same with device pointers for values, group, out and counts, on the context's stream under the vcp_set_stream contract;
 * q stays a host pointer.  One synchronisation before the outputs are touched (the label check); returns when the result
 * is in place. */
int vcp_cluster_quantiles_dev(vcp_ctx* ctx, const double* d_values, int64_t stride, const int32_t* d_group, int64_t n,
                              int32_t K, const double* q, int32_t nq, double* d_out, int64_t* d_counts);
int vcp_cluster_mad(vcp_ctx* ctx, const double* values, int64_t stride, const int32_t* group, int64_t n, int32_t K,
                    double c_mad, double floor, double* med, double* mad, double* thr, uint8_t* reject, int64_t* kept,
                    int64_t* n_rejected);
/* Same with device pointers for values, group, med, mad, thr, reject and kept; n_rejected stays a host pointer. */
int vcp_cluster_mad_dev(vcp_ctx* ctx, const double* d_values, int64_t stride, const int32_t* d_group, int64_t n,
                        int32_t K, double c_mad, double floor, double* d_med, double* d_mad, double* d_thr,
                        uint8_t* d_reject, int64_t* d_kept, int64_t* n_rejected);
/* Self-test of the key and the rank, compiled from the same __host__ __device__ source as the kernels: *key = key(v),
 * *rank = the rank of q in a group of c rows.  Returns 1, or VCP_ERR_ARG for a NULL pointer, c < 1, or q that is NaN or
 * outside [0, 1].  Needs no device and no context. */
int vcp_selftest_rank_key(double v, double q, int64_t c, uint64_t* key, int64_t* rank);

/* -- per-cluster covariance, principal axes and the ellipse numbers -----------------------------------------
 * vcp_cluster_shapes describes a cluster by extreme values (hull, circle, rectangle): one stray point moves them by its full
 * distance, a hull beyond 2048 points fails the call, a cluster of <= 3 points is not judged, and it is 2-D only.  The second
 * central moments have none of these limits: per cluster the mean, the population covariance, its eigenvalues and principal
 * axes, and four numbers derived from them.  2 sqrt(lambda) is the radius of a uniformly filled disc (variance r^2 / 4 on
 * every axis); in 3-D the axis of the smallest eigenvalue is the surface normal and lambda_3 / (lambda_1 + lambda_2 +
 * lambda_3) measures how flat the cluster is.  The outputs feed vcp_cluster_filter as they stand (radius = 2 shape[0],
 * rect_len = 2 (shape[0], shape[1]), valid for both flags).
 *   pts        row i is pts[i * ld + 0 .. dim), dim = 2 or 3, ld >= dim in doubles: xyz[:, :2], motor, or columns of a
 *              wider resident array are read in place
 *   labels     [n] in 0..K, 0 = in no cluster
 *   weights    [n] int32 >= 0 (the count of vcp_import_compact), or NULL for 1
 * Definition.  All arithmetic binary64, every operation rounded on its own (no FMA contraction), / and sqrt correctly
 * rounded.  The members of cluster k in ascending point index; every sum below through the fixed tree of vcp_centroids:
 * chunks of 16384 consecutive members, in a chunk 256 threads strided (thread t adds members t, t + 256, ... from +0.0),
 * per wave of 64 the shuffle tree at offsets 32, 16, 8, 4, 2, 1, the 4 waves in order, the chunks in order from 0.0.
 *   1. W      = sum w                                       integers: exact; (double)W below
 *   2. m_a    = (sum fl(w x_a)) / W                         with weights == NULL: vcp_centroids' mean of the same numbers, bit
 *                                                           for bit (1.0 * x is x)
 *   3. d_a    = fl(x_a - m_a);  p_ab = fl(fl(w d_a) d_b)    a <= b; with no weights fl(d_a d_b), the same bits
 *   4. S_ab   = sum p_ab;  cov_ab = S_ab / W                the population covariance, one division
 *   5. eval, evec = the eigen-solve of cov by csrc/symeig.hpp (cyclic Jacobi; the operation sequence is in its header):
 *               eigenvalues descending, equal ones in the order of their diagonal position; eigenvector j is ROW j of evec,
 *               its component of largest magnitude (the first such) positive, so det(evec) may be -1; a non-finite entry
 *               of cov gives NaN in all of eval and evec; an all-zero cov gives +0 and the identity; a negative computed
 *               eigenvalue (rounding, a rank-deficient cluster) is reported as computed
 *   6. shape  = (sigma_max, sigma_min_inplane, flatness, tilt): sigma = sqrt(eval > 0 ? eval : 0) of eval[0] and eval[1];
 *               flatness = eval[2] / ((eval[0] + eval[1]) + eval[2]), 0 when that sum is 0, and +0 for dim 2;
 *               tilt = fabs(evec[2][2]), the z-component of the last axis, and 1 for dim 2; all four NaN where eval is NaN
 * The sums are centred, in two passes, on purpose: a cloud at 1e8 from the origin loses every digit of a covariance formed
 * from raw moments (DESIGN.md section 33 has the bound of this form and the counter-example).
 * Outputs, each of which may be NULL: mean [K*dim]; cov [K*dim(dim+1)/2] packed by rows of the upper triangle, (xx, xy, yy)
 * or (xx, xy, xz, yy, yz, zz); eval [K*dim]; evec [K*dim*dim]; shape [K*4]; valid [K] = 1 when W >= 2 and every entry of
 * mean and cov is finite; counts [K] = W.  A NaN is written as 0x7FF8000000000000.
 *   a cluster without members, or of total weight 0:   counts 0, valid 0, NaN in every double output (0 / 0)
 *   total weight 1:                                     cov +0 (for a finite point), eval +0, evec the identity, valid 0
 * Errors, found before any output is touched; nothing is written on an error.  VCP_ERR_ARG: NULL ctx, n < 0, K < 0, dim not
 * 2 or 3, ld < dim, NULL pts or labels with n > 0, a negative weight (found on the device); VCP_ERR_INDEX: a label outside
 * 0..K (found on the device); VCP_ERR_TOO_LARGE: n >= 0x7FFFFFF0, as vcp_centroids_dev.  K == 0 or n == 0: nothing to sum;
 * the outputs for K > 0 are the empty-cluster values, VCP_OK.
 * Every cluster takes the same road whatever its size (chunk partials, then one thread per cluster), and the result is a
 * function of the input alone: two calls give identical bits, and so does a call after any other call on the context.
 * Timing phases: moments_group, moments_mean, moments_cov (csrc/cluster_moments.hip). */
int vcp_cluster_moments(vcp_ctx* ctx, const double* pts, int64_t ld, int dim, const int32_t* labels,
                        const int32_t* weights, int64_t n, int32_t K, double* mean, double* cov, double* eval,
                        double* evec, double* shape, uint8_t* valid, int64_t* counts);
/* Same with device pointers, on the context's stream under the vcp_set_stream contract.  One synchronisation before the
 * outputs are touched (the label and weight check); returns when the result is in place. */
int vcp_cluster_moments_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int dim, const int32_t* d_labels,
                            const int32_t* d_weights, int64_t n, int32_t K, double* d_mean, double* d_cov,
                            double* d_eval, double* d_evec, double* d_shape, uint8_t* d_valid, int64_t* d_counts);
/* The eigen-solve of step 5 on the host, compiled from the same __host__ __device__ source as the kernel: s_packed holds the
 * upper triangle by rows (3 or 6 doubles), eval [dim], evec [dim*dim]; *sweeps (may be NULL) = the Jacobi sweeps made.
 * Returns 1, or VCP_ERR_ARG for a NULL s_packed, eval or evec or a dim that is not 2 or 3.  Needs no device and no
 * context. */
int vcp_selftest_sym_eig(int dim, const double* s_packed, double* eval, double* evec, int* sweeps);

/* -- per-cluster least-squares sphere (3-D) and circle (2-D) fit ---------------------------------------------
 * The instrument is the origin of X, Y, Z (vcp_import_convert), so a target is seen from one side: the mean of the returns
 * of a sphere of radius R lies about 2R/3 in front of its centre, on the line to the instrument, and a half-hidden disc has
 * its mean in the visible half.  Taken over a field these shifts are a radial shrink, which no rigid fit absorbs.  The
 * least-squares fit gives the centre the returns lie around, with the radius free or fixed to the known target radius, and
 * a radius, a residual and a coverage number to judge the cluster by.
 *   pts, ld, dim, labels, weights     exactly as in vcp_cluster_moments (dim 2: circle, dim 3: sphere)
 *   fixed_radius   0: the radius is fitted; finite and > 0: it is this value
 *   rounds         Gauss-Newton rounds, 0..64
 * Definition.  All arithmetic binary64, every operation rounded on its own (no FMA contraction), / and sqrt correctly
 * rounded.  The members of cluster k in ascending point index; every sum through the fixed tree of vcp_centroids, as stated
 * for vcp_cluster_moments.  x . y for vectors of dim 2 is fl(fl(x0 y0) + fl(x1 y1)), of dim 3 fl(that + fl(x2 y2)).
 *   1. W, m, d_a = fl(x_a - m_a)      steps 1 to 3 of vcp_cluster_moments: counts and m are its bits.  Everything below works
 *                                     on d and on u = c - m, never on raw coordinates: a field at 1e8 keeps its digits
 *   2. the algebraic start (Kasa, centred):
 *        S_ab = sum fl(fl(w d_a) d_b)  (a <= b; vcp_cluster_moments' S);   q = d . d;   T_a = sum fl(fl(w q) d_a)
 *        u0   = the solution of S u0 = h, h_a = fl(T_a * 0.5), by csrc/spdsolve.hpp (L D L^T; the operation sequence is in
 *               its header; it fails when a pivot is not finite and > 0)
 *        r0   = sqrt(fl(u0 . u0 + fl(tr / W))),  tr = fl(S_00 + S_11), for dim 3 fl(that + S_22)
 *        alg  = (fl(m_a + u0_a), r0);   u = u0;   r_ref = fixed_radius > 0 ? fixed_radius : r0
 *   3. `rounds` times, on the residual rho_i - r:
 *        e = fl(d - u);  rho = sqrt(e . e);  nu_a = fl(e_a / rho), and nu = 0 for a member with rho == 0: it lies on the
 *        current centre, has no direction, and adds fl(w * 0) to every sum with nu in it
 *        N_ab = sum fl(fl(w nu_a) nu_b) (a <= b);  b_a = sum fl(w nu_a);  R = sum fl(w rho);  g_a = sum fl(fl(w rho) nu_a)
 *        free:   M_ab = fl(N_ab - fl(fl(b_a b_b) / W));  y_a = fl(g_a - fl(fl(R b_a) / W));  r_ref = fl(R / W)
 *        fixed:  M = N;                                  y_a = fl(g_a - fl(fixed_radius * b_a))
 *        delta = the solution of M delta = y (spdsolve.hpp);   u_a = fl(u_a + delta_a);   step = sqrt(delta . delta)
 *      The free form is the normal equations of (u, r) with r eliminated.  delta = +M^-1 y: the other sign diverges.
 *   4. the closing pass, at the last u:  e, rho, nu as in 3;  c = fl(rho - r_ref)
 *        b_a = sum fl(w nu_a);   C1 = sum fl(w c);   C2 = sum fl(fl(w c) c);   cbar = fl(C1 / W)
 *        free:   radius = fl(r_ref + cbar)  (= sum w rho / W, summed around r_ref, the radius the last round saw, or r0);
 *                rms = sqrt(max(fl(fl(C2 / W) - fl(cbar cbar)), 0))
 *        fixed:  radius = fixed_radius;   rms = sqrt(fl(C2 / W))
 *        centre_a = fl(m_a + u_a);   cap = fl(sqrt(b . b) / W);   step = the last round's (0 for rounds == 0)
 *      rms is formed from the centred c, never from sum rho^2 - ...  cap tells how much of the target was seen: about 0
 *      for a whole sphere, 2/3 for a cap seen from afar, towards 1 for a sliver, where the fit is ill-conditioned.
 *   5. valid = 1 when W >= dim + 1 (free) or W >= dim (fixed), no solve of the call failed for the cluster, and every double
 *      output of the cluster is finite.  An invalid cluster has NaN (0x7FF8000000000000) in every double output and keeps
 *      its counts: too few members, coincident, collinear or (dim 3) coplanar members (a pivot of 0), a non-finite
 *      coordinate, a cluster without members or of total weight 0 (counts 0).  Once a solve fails the cluster stays invalid;
 *      every cluster runs every round, and nothing the host decides depends on the data after the label and weight check.
 * Outputs, each of which may be NULL: centre [K*dim]; radius, rms, cap, step [K]; alg [K*(dim+1)]; valid [K]; counts [K] = W.
 * Errors, found before any output is touched; nothing is written on an error.  Those of vcp_cluster_moments, and
 * VCP_ERR_ARG for a fixed_radius that is negative, NaN or infinite and for rounds outside 0..64; VCP_ERR_NOMEM when the
 * workspace of n * (8 dim + 4) bytes cannot be had (there is no second road).  K == 0 or n == 0 as in vcp_cluster_moments.
 * The result is a function of the input alone: two calls give identical bits, and so does a call after any other call on
 * the context.  Timing phases: spheres_group, spheres_start, spheres_rounds (csrc/cluster_spheres.hip, DESIGN.md section
 * 34). */
int vcp_cluster_spheres(vcp_ctx* ctx, const double* pts, int64_t ld, int dim, const int32_t* labels,
                        const int32_t* weights, int64_t n, int32_t K, double fixed_radius, int rounds, double* centre,
                        double* radius, double* rms, double* cap, double* step, double* alg, uint8_t* valid,
                        int64_t* counts);
/* Same with device pointers, on the context's stream under the vcp_set_stream contract.  One synchronisation before the
 * outputs are touched (the label and weight check); returns when the result is in place. */
int vcp_cluster_spheres_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int dim, const int32_t* d_labels,
                            const int32_t* d_weights, int64_t n, int32_t K, double fixed_radius, int rounds,
                            double* d_centre, double* d_radius, double* d_rms, double* d_cap, double* d_step,
                            double* d_alg, uint8_t* d_valid, int64_t* d_counts);
/* The solve of steps 2 and 3 on the host, compiled from the same __host__ __device__ source as the kernels: s_packed holds
 * the upper triangle by rows (3 or 6 doubles), b and x [dim]; *ok (may be NULL) = 1, or 0 when a pivot was not finite and
 * > 0 (x is then NaN).  Returns 1, or VCP_ERR_ARG for a NULL s_packed, b or x or a dim that is not 2 or 3 (nothing is
 * written).  Needs no device and no context. */
int vcp_selftest_spd_solve(int dim, const double* s_packed, const double* b, double* x, int* ok);

/* -- scan text on the device: bytes in, resident rows out --------------------------------------------------
 * The reference's scan files hold one point per line, `motor_x<TAB>motor_y<TAB>Distance` (FileMap.ReadFile,
 * FrmMain.cs:1005-1009; written back by BC/Tools.cs:233).  The bytes of one or many files go in; rows [n, 3] and the file
 * number of every row come out in the layout vcp_import_compact_dev(d_rows, d_group) takes.  In BOTH forms text is a HOST
 * buffer; "_dev" means that d_rows [cap * 3] and d_group [cap] are device pointers, written on the context's stream under
 * the vcp_set_stream contract.  group may be NULL.  The result equals vtkcloudpoint_amd.io.read_scan_text bit for bit.
 *   segments   seg_off [nseg + 1] ascends from seg_off[0] = 0 to seg_off[nseg] = nbytes; segment k is file k; seg_off ==
 *              NULL means one segment (nseg is not read).  Every non-empty segment must end with '\n' (nseg byte reads on
 *              the host; else VCP_ERR_ARG): no line and no "\r\n" pair then spans two files
 *   bytes      \t \n \r and 0x20..0x7E except '_'.  Any other byte: VCP_ERR_UNSUPPORTED with err[0] = the offset of the first
 *              one (a device minimum).  On those bytes a reader in Python differs from any simple grammar (GB2312 pairs,
 *              str.splitlines on 0x0B 0x0C 0x1C-0x1E 0x85, 1_0 == 10); callers fall back to their own reader
 *   lines      the terminators are "\r\n", '\n' and a '\r' that no '\n' follows; *n = their number; an empty line between
 *              two terminators is a line.  seg_first [nseg + 1] (may be NULL) = the first line of every segment;
 *              group[j] = the segment that holds the first byte of line j
 *   fields     a line is split at '\t'; the first three fields are read, further fields are ignored whatever they hold
 *   a number   sp* [+-]? (D+ ('.' D*)? | '.' D+) ([eE] [+-]? D+)? sp*  (D a decimal digit, sp a blank), or inf, infinity,
 *              nan with an optional sign in any letter case: what Python's float() accepts on supported bytes.  The value
 *              is the correctly rounded binary64 (nearest, ties to even); -0 gives -0.0; nan and +nan give
 *              0x7FF8000000000000, -nan gives 0xFFF8000000000000
 *   classes    with w the mantissa's digits as an integer (leading zeros stripped, trailing zeros counted), nd the number
 *              of those digits and e10 the exponent minus the number of fraction digits (vcp_selftest_parse_field
 *              returns the class):
 *                1  w == 0, or w <= 2^53 and -22 <= e10 <= 22: (double)w * 1e{e10} or (double)w / 1e{-e10}, one IEEE
 *                   operation on an exact power (Clinger's fast path)
 *                2  otherwise nd <= 19 and -19 <= e10 <= 19: w * 10^e10 in integers -- an exact 128-bit product, or a
 *                   128-by-64-bit long division with a sticky bit -- rounded by hand
 *                3  any other number (more digits, larger exponents, the names): parsed on the host, locale-independent
 *                   and correctly rounded
 *                0  not a number
 *              Classes 1 and 2 are decided and evaluated on the device.  The lines with a class-3 field go to a list the
 *              library sorts; it parses them from text on the host and patches rows with one upload and one scatter
 *              kernel on the context's stream.  *n_host = the number of such lines
 *   errors     the first line, in input order, with fewer than three fields (kind 1) or a non-number among its first three
 *              fields (kind 2; the field count is checked first): VCP_ERR_ARG with err = {line within its segment
 *              (1-based), segment, kind}.  *n and *n_host are then NOT written and the contents of rows and group are
 *              unspecified: validating before writing would mean parsing twice.  err may be NULL
 *   counting   rows == NULL (d_rows == NULL): count-only -- the bytes and the segment rule are checked, *n and seg_first
 *              are written, nothing is parsed.  n > cap: VCP_ERR_INDEX, and *n IS written, so that the caller can come
 *              back with room
 * Limits: nbytes >= 2^32 or n >= 0x7FFFFFF0: VCP_ERR_TOO_LARGE.  nbytes == 0: *n = 0, VCP_OK.  VCP_ERR_ARG also for a
 * NULL ctx, n or text (nbytes > 0), nseg < 1 with a seg_off, cap < 0.
 * The result is a function of the input alone: integer minima, and a list that is sorted before use, are the only
 * atomics that decide anything.  Workspace: the text, 4 bytes per VCP_TXT_CHUNK bytes, 12 bytes per line.  Timing phases:
 * txt_upload, txt_index, txt_parse, txt_patch (csrc/scantext.hip, csrc/scantext.hpp). */
#define VCP_TXT_CHUNK 16384 /* bytes one workgroup indexes */
int vcp_parse_scan_text(vcp_ctx* ctx, const char* text, uint64_t nbytes, const uint64_t* seg_off, int32_t nseg, int64_t cap,
                        double* rows, int32_t* group, int64_t* seg_first, int64_t* n, int64_t* n_host, int64_t err[3]);
int vcp_parse_scan_text_dev(vcp_ctx* ctx, const char* text, uint64_t nbytes, const uint64_t* seg_off, int32_t nseg,
                            int64_t cap, double* d_rows, int32_t* d_group, int64_t* seg_first, int64_t* n,
                            int64_t* n_host, int64_t err[3]);
/* One field through the source the kernels compile (csrc/scantext.hpp): returns the class; for classes 1..3 *v = the
 * value (class 3 through the host's parser), for class 0 *v is untouched.  VCP_ERR_ARG for a NULL v, len < 0 or a NULL s
 * with len > 0.  Needs no device and no context. */
int vcp_selftest_parse_field(const char* s, int64_t len, double* v);

/* -- export text on the device: resident rows in, the file's bytes out ------------------------------------
 * The inverse of vcp_parse_scan_text: the lines the reference's exports write one Point3D at a time (BC/Tools.cs:233, 295,
 * 341, 374: the filtered scan, the cluster export, the centroid export), built from columns that stay where they are.
 *   line j     [id[r] TAB] a[r * stride_a] TAB b[r * stride_b] TAB c[r * stride_c] EOL with r = order[j], j = 0..m-1;
 *              order == NULL: r = j, and m must equal n.  id == NULL: no id column.  Strides are in doubles, >= 1: the
 *              columns of one [n, 3] array (stride 3), separate arrays, or the same array three times, all read in place.
 *              eol 0 = "\n", 1 = "\r\n"
 *   a number   the bytes of Python's '%.*f' % (bit, v), 0 <= bit <= 15: the exact binary value rounded to `bit` decimals,
 *              ties to even; '-' whenever the sign bit is set (-0.0 and -1e-9 give -0.000000); no decimal point at
 *              bit == 0; no leading zeros but the single 0.  Supported: v finite, |v| < 1e15.  An id prints as '%d'
 *   order      m entries, repeats and subsets allowed.  The first j whose entry is outside [0, n): VCP_ERR_INDEX with
 *              err = {j, entry}
 *   text       a HOST buffer of cap bytes in BOTH forms; "_dev" means that d_id, d_a, d_b, d_c and d_order are device
 *              pointers, read on the context's stream under the vcp_set_stream contract.  The bytes are built in the
 *              workspace and copied down.  *nbytes is written whenever the inputs are valid; text == NULL is count-only;
 *              *nbytes > cap: VCP_ERR_INDEX with *nbytes written, so that the caller can come back with room, text untouched
 *   unsupported  the first line j, in output order, that holds a NaN, an infinity or a magnitude >= 1e15, and its first
 *              such column: VCP_ERR_UNSUPPORTED with err = {j, column 0..2} (an integer device minimum); text untouched,
 *              *nbytes not written.  There is no approximation and no host fallback in the library: callers format such a
 *              call themselves.  A bad entry of order is reported before an unsupported value
 * No line is longer than VCP_FMT_LINE_MAX bytes: an 11-byte id, three fields of at most 32 bytes ('-', 15 digits, '.',
 * 15 digits: 10^15 itself appears only at bit 0, as 16 digits without a point), three tabs and "\r\n".
 * Limits: a text of 2^32 bytes or more: VCP_ERR_TOO_LARGE, found from the exact 64-bit byte count.  m == 0: *nbytes = 0,
 * VCP_OK.  VCP_ERR_ARG: NULL ctx, NULL nbytes, a NULL column with m > 0, a stride < 1, bit outside 0..15, eol outside
 * 0..1, n < 0, m < 0, order == NULL with m != n.  err may be NULL.
 * The result is a function of the input alone: integer minima are the only atomics that decide anything.  Workspace: 4
 * bytes per 256 lines and the text (the host form: its inputs as well).  Timing phases: fmt_len, fmt_write, fmt_download
 * (csrc/scanfmt.hip, csrc/scanfmt.hpp). */
#define VCP_FMT_LINE_MAX 112
int vcp_format_rows(vcp_ctx* ctx, const int32_t* id, const double* a, int64_t stride_a, const double* b, int64_t stride_b,
                    const double* c, int64_t stride_c, const int64_t* order, int64_t n, int64_t m, int bit, int eol,
                    char* text, uint64_t cap, uint64_t* nbytes, int64_t err[2]);
int vcp_format_rows_dev(vcp_ctx* ctx, const int32_t* d_id, const double* d_a, int64_t stride_a, const double* d_b,
                        int64_t stride_b, const double* d_c, int64_t stride_c, const int64_t* d_order, int64_t n, int64_t m,
                        int bit, int eol, char* text, uint64_t cap, uint64_t* nbytes, int64_t err[2]);
/* One number through the source the kernels compile (csrc/scanfmt.hpp): returns 1 with the field's bytes in out (no
 * terminator) and their number in *len, or 0 for an unsupported v, nothing written.  VCP_ERR_ARG for a NULL out or len, bit
 * outside 0..15, or cap smaller than the field (*len is written then, out is not).  Needs no device and no context. */
int vcp_selftest_format_field(double v, int bit, char* out, int64_t cap, int64_t* len);
/* The 64-bit sum vcp_format_rows takes its byte count from, run on n words the caller supplies (a device pointer). */
int vcp_selftest_format_total_dev(vcp_ctx* ctx, const uint32_t* d_totals, int64_t n, uint64_t* total);

/* Self-test of the wave and workgroup idioms the kernels share (csrc/wave.hpp): ONE workgroup of tb
 * threads (64, 256, 512 or 1024) over d_words [n] and d_flags [n], 0 <= n <= tb; thread t holds v = d_words[t] and
 * p = d_flags[t] != 0, and v = 0, p = false from t = n on.  d_out [VCP_WAVE_ROWS][tb], row r of thread t, sums modulo 2^32:
 *    0  the sum of v over the threads before t          1  the same, from the form that also returns  2  the sum over all
 *    3, 4, 5  sum, minimum, maximum of v over t's wave   6  the OR of v over t's wave (through the 64-bit form)
 *    7  the p threads of t's wave                        8  the p threads of the workgroup in thread 0, 0xFFFFFFFF elsewhere
 *    9, 10  the same for p and for odd v, from the two-predicate form
 *   11  p: the p threads before t; otherwise 0          12  the p threads before t   13  the p threads of the workgroup
 *   14  p: t's slot from the wave-aggregated append on *d_counter, which the caller has set to a start value and which
 *       ends at start + the p threads; otherwise 0xFFFFFFFF
 *   15  the maximum of v over the lanes of t's wave up to t   16  the sum of v over the lanes of t's half-wave up to t
 *   17  v of thread t - 1 (of t itself in lane 0 of a wave)
 *   18 .. 23  with s = (v - 2^31) * 2^20 as a signed 64-bit integer: low and high word of the sum (modulo 2^64), of the
 *       maximum and of the minimum of s over t's wave
 * Device pointers; returns when d_out is in place.  VCP_ERR_ARG: another tb, n outside [0, tb], a NULL pointer. */
#define VCP_WAVE_ROWS 24
int vcp_selftest_wave_dev(vcp_ctx* ctx, const uint32_t* d_words, const uint8_t* d_flags, int64_t n, int tb,
                          uint32_t* d_counter, uint32_t* d_out);

#ifdef __cplusplus
}
#endif
#endif
