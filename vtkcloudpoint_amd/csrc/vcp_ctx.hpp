// vcp_ctx.hpp -- context, workspace and error plumbing shared by the libvcp.so translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "vcp.h"

// A growable device buffer owned by the context (no hipMalloc on the steady-state path).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool registered = false;  // listed in vcp_ctx::bufs (exactly once, whatever happens to p afterwards)
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

struct Phase {
  const char* name;
  hipEvent_t ev;  // recorded BEFORE the phase starts
};

struct vcp_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  hipDeviceProp_t prop;
  // pinned scratch for tiny readbacks (64 KB).  Who reads back where (byte offsets; a context runs one call at a time on
  // one stream, and every user has consumed its words before the call that wrote them returns or goes on):
  //   [0, 1024)     the DBSCAN engine's EnginePinned: bounds, two totals, counters (dbscan.hip); the block partition's bounds (blockpart.hip);
  //                 the finish stage's counters (blocks.hip); the k-distance bounds (kdist.hip); at [512, 568) the
  //                 nearest-neighbour grid's bounds (nngrid.hip); at [0, 56) the truths' bounds of vcp_match_unique
  //                 and the targets' bounds of vcp_register_pairs (epsgrid.hpp) and the cloud's of vcp_eps_tree (eps_tree.hip);
  //                 at [0, 128) the weight check and the bounds of vcp_gdbscan (gdbscan.hip); at [0, 72) the counters of
  //                 vcp_cluster_quantiles / vcp_cluster_mad and at [128, 264) their ranks on the way up (cluster_quant.hip);
  //                 at [0, 24) the counters of vcp_parse_scan_text (scantext.hip); at [0, 32) those of vcp_format_rows
  //                 (scanfmt.hip); at [0, 32) the counters of vcp_cluster_moments and vcp_cluster_spheres (cluster_seg.hpp)
  //   [1024, 2048)  the partition's SelState (blockpart.hip); the all-pairs kernel's counters (blocks.hip: blocks_cluster);
  //                 DB's counters (dbdead.hip, dbpairs.hip); the round counters of vcp_match_unique (match_unique.hip)
  //                 and of vcp_eps_tree (eps_tree.hip); the cluster count of vcp_gdbscan (gdbscan.hip)
  //   [2048, 2064)  DB pair by pair: next seed / frontier size (dbpairs.hip)
  //   [4096, 4224)  plane extraction (planes.hip): m, the winner, the refit's count and plane, the rows labelled.  Clear of
  //                 [0, 32), which the refit's vcp_cluster_moments_dev writes between them
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  // pinned staging area of the host-buffer entry points with several small arrays (vcp_stage; grown on demand, <= 64 MiB)
  void* stage = nullptr;
  size_t stage_bytes = 0;
  uint32_t scan_gen = 0;  // generation number of the scan descriptors in b_scan_tmp (vcp_ctx.hip: k_scan)
  // vcp_selftest_poison (vcp_ctx.hip): while armed, every fresh allocation is filled with the word before first use
  bool poison_armed = false;
  uint32_t poison_word = 0;
  // workspace
  std::vector<DevBuf*> bufs;
  DevBuf b_cellof, b_rank, b_sidx, b_flags, b_parent, b_minord, b_seedflag,
      b_rootcl, b_clseed, b_scan_tmp, b_misc, b_in0, b_in1, b_in2, b_in3, b_out0, b_out1, b_out2,
      b_out3, b_icp_part, b_aux0, b_aux1, b_aux2, b_aux3, b_aux4, b_aux5, b_pos, b_labk, b_sgroup, b_wl, b_hist, b_rec, b_nn_misc, b_nn_cells, b_nn_cid, b_nn_rec, b_nn_cur, b_nbr, b_nboff, b_sorted32, b_self, b_outcur, b_fineq, b_rec2, b_bstart, b_ctw, b_ctd, b_bstate;
  // k-distance (kdist.hip)
  DevBuf b_kd_in, b_kd_out, b_kd_outk, b_kd_part, b_kd_key, b_kd_val, b_kd_rec, b_kd_start, b_kd_heavy, b_kd_tmp;
  // cluster shapes and the cluster filter (shapes.hip): hull points per member slot, the host forms' rectangle / hull /
  // filter outputs, the filter's keep flags and their scan
  DevBuf b_sh_hull, b_sh_out, b_sh_flag;
  // one-to-one matching (match_unique.hip): per-centroid state, per-truth state and the truths cell by cell, the round
  // counters and the bounds, the cell starts of its own truth grid
  DevBuf b_mu_cent, b_mu_truth, b_mu_misc, b_mu_cell;
  // congruent-pair registration (register.hip): source, targets and bases of the host form; the targets cell by cell; the
  // cell starts of its own target grid; the base table, the winners' words and the per-base results
  DevBuf b_rg_in, b_rg_truth, b_rg_cell, b_rg_work;
  // eps tree (eps_tree.hip): inputs and outputs of the host form; its own k-distances; counters and bounds; the cell
  // starts of its own grid; the records and per-slot state; the emitted edges and the sort's second set; the sort's
  // temporary storage
  DevBuf b_et_in, b_et_out, b_et_kd, b_et_misc, b_et_cell, b_et_work, b_et_edge, b_et_tmp;
  // weighted / gated DBSCAN (gdbscan.hip): inputs and outputs of the host form; counters and bounds; the cell starts of
  // its own grid; the records, the per-slot state and the ranks
  DevBuf b_gd_in, b_gd_out, b_gd_misc, b_gd_cell, b_gd_work;
  // trimmed ICP (icp.hip): per (pose, landmark) the distance key and the index found, then the select's prefixes and
  // histograms; unique-correspondence ICP: the same keys and indices, then per (pose, target) the winner's slot
  DevBuf b_icpt;
  // per-cluster quantiles and MAD (cluster_quant.hip): values and groups, then the outputs, of the host forms; the segment
  // tables, counters and ranks; the large segments' select states and histograms.  The keys in segment order are b_aux4
  DevBuf b_cq_in, b_cq_out, b_cq_misc, b_cq_large;
  // scan text (scantext.hip): the copy of the text; one word per chunk; counters, seg_off and seg_first; line_start and
  // the host list; rows and group of the host form; the host-parsed values on their way up
  DevBuf b_tx_text, b_tx_chunk, b_tx_misc, b_tx_line, b_tx_out, b_tx_patch;
  // export text (scanfmt.hip): columns, ids and order of the host form; one word per workgroup; counters; the text
  DevBuf b_fm_in, b_fm_wg, b_fm_misc, b_fm_text;
  // per-cluster moments (cluster_moments.hip): points, labels and weights, then the outputs, of the host form; the segment
  // tables, the counters, and per cluster the total weight and the mean.  The chunk partials are b_aux4
  DevBuf b_cm_in, b_cm_out, b_cm_misc;
  // per-cluster sphere / circle fit (cluster_spheres.hip): points, labels and weights, then the outputs, of the host form;
  // the same tables as b_cm_misc with the per-cluster fit state behind them; the centred rows d (one plane per coordinate)
  // and the weights in (label, index) order, which every round streams.  The chunk partials are b_aux4
  DevBuf b_cs_in, b_cs_out, b_cs_misc, b_cs_d;
  struct BlocksState* blocks = nullptr;  // staged block-partitioned pipeline (blocks.hip)
  struct SlabState* slab = nullptr;      // staged exact multi-GPU DBSCAN (dbscan.hip: vcp_slab_*)
  // plane extraction (planes.hip, which describes them): its workspace buffers b_pl_*.  They are listed in `bufs` like
  // the members above (freed with the workspace, filled by vcp_selftest_poison); the struct itself goes with the context
  struct PlanesWs* planes = nullptr;
  struct FeaturesWs* features = nullptr;  // per-point features (point_features.hip): b_pf_*, held the same way
  // timing
  bool timing = false;
  std::vector<Phase> phases;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<std::pair<const char*, float>> last_timing;
};

int vcp_fail(vcp_ctx* ctx, int code, const char* fmt, ...);
// pinned host memory of at least `bytes` (nullptr when bytes > 64 MiB or the allocation fails: callers then copy
// array by array from the caller's pageable memory)
void* vcp_stage(vcp_ctx* ctx, size_t bytes);

#define VCP_HIP(ctx, call)                                                                    \
  do {                                                                                        \
    hipError_t e__ = (call);                                                                  \
    if (e__ != hipSuccess)                                                                    \
      return vcp_fail((ctx), VCP_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,        \
                      hipGetErrorString(e__));                                                \
  } while (0)

#define VCP_TRY(expr)        \
  do {                       \
    int rc__ = (expr);       \
    if (rc__ != VCP_OK) return rc__; \
  } while (0)

// ensure capacity (contents are NOT preserved).  listed: the context frees the buffer on destroy (vcp_ctx::bufs); a
// buffer owned by some other state, which frees it itself, passes false.
int vcp_ensure(vcp_ctx* ctx, DevBuf& b, size_t bytes, bool listed = true);
// bind the calling thread to the context's device
int vcp_bind(vcp_ctx* ctx);
// timing
void vcp_phase_reset(vcp_ctx* ctx);
void vcp_phase(vcp_ctx* ctx, const char* name);  // marks the start of a phase
int vcp_phase_finish(vcp_ctx* ctx);              // closes the last phase, syncs, fills last_timing

constexpr unsigned vcp_blocks(int64_t n, int per_block, int cap = 1 << 30) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// Whether the runtime can represent a dispatch of `grid` workgroups of `block` threads with `lds` bytes of dynamic LDS.
// It does not refuse more than 2^32 - 1 work-items on an axis: it wraps the count and dispatches fewer workgroups.  The
// LDS limit is gfx950's 160 KB (beyond 64 KB a kernel has to be allowed through hipFuncSetAttribute).
constexpr bool vcp_launch_ok(dim3 grid, dim3 block, size_t lds) {
  return grid.x >= 1 && grid.y >= 1 && grid.z >= 1 && block.x >= 1 && block.y >= 1 && block.z >= 1 &&
         (uint64_t)grid.x * block.x <= 0xFFFFFFFFu && (uint64_t)grid.y * block.y <= 0xFFFFFFFFu &&
         (uint64_t)grid.z * block.z <= 0xFFFFFFFFu && block.x <= 1024 && block.y <= 1024 && block.z <= 1024 &&
         (uint64_t)block.x * block.y * block.z <= 1024 && lds <= 160 * 1024;
}
static_assert(vcp_launch_ok(dim3((1u << 24) - 1), dim3(256), 0) && !vcp_launch_ok(dim3(1u << 24), dim3(256), 0));
static_assert(vcp_launch_ok(dim3(1), dim3(1024), 0) && !vcp_launch_ok(dim3(1), dim3(1025), 0));
static_assert(vcp_launch_ok(dim3(1), dim3(64), 163840) && !vcp_launch_ok(dim3(1), dim3(64), 163841));
static_assert(!vcp_launch_ok(dim3(0), dim3(64), 0) && !vcp_launch_ok(dim3(1, 1, 0), dim3(64), 0) &&
                  !vcp_launch_ok(dim3(1), dim3(64, 0), 0));

// The launch and decision trace (VCP_TRACE set to anything but empty or 0; read once per process; off by default).  When it
// is on, every VCP_LAUNCH writes `vcp-trace launch <kernel>` to stderr before the launch -- <kernel> is the macro's kernel
// argument as written, whitespace collapsed, e.g. `k_flatten0<2>` or `(k_union<GD, METRIC, GROUPED, true, true>)` -- and
// the host drivers write one `vcp-trace <what> key=value ...` line where they choose between paths (vcp_trace_line).
// Each line is ONE unbuffered write, so it interleaves cleanly with whatever else the process writes there.  The tests
// (tests/test_engine_paths_gpu.py) read the path a call took from these lines.
bool vcp_trace_on();
void vcp_trace_launch(const char* kernel);
void vcp_trace_line(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// Launches `kernel` (grid, block, dynamic LDS bytes, stream, arguments) in a function that returns a vcp status: a
// dispatch that vcp_launch_ok refuses is VCP_ERR_TOO_LARGE before anything is enqueued, a launch error VCP_ERR_HIP, both
// naming the kernel.  grid, block and lds are evaluated once; a templated kernel stays in parentheses.
#define VCP_LAUNCH(ctx, kernel, grid, block, lds, stream, ...)                                                         \
  do {                                                                                                                 \
    const dim3 g__ = (grid), b__ = (block);                                                                            \
    const size_t l__ = (lds);                                                                                          \
    if (!vcp_launch_ok(g__, b__, l__))                                                                                 \
      return vcp_fail((ctx), VCP_ERR_TOO_LARGE, "%s: grid %ux%ux%u, block %ux%ux%u, lds %zu", #kernel, g__.x, g__.y,   \
                      g__.z, b__.x, b__.y, b__.z, l__);                                                                \
    if (__builtin_expect(vcp_trace_on(), 0)) vcp_trace_launch(#kernel);                                                \
    hipLaunchKernelGGL(kernel, g__, b__, l__, stream, __VA_ARGS__);                                                    \
    const hipError_t e__ = hipGetLastError();                                                                          \
    if (e__ != hipSuccess) return vcp_fail((ctx), VCP_ERR_HIP, "%s: %s", #kernel, hipGetErrorString(e__));             \
  } while (0)

// exclusive scan of n uint32 (in place allowed: out may equal in); writes the grand total to
// d_total (device uint32) if non-null.  Defined in scan.hip.
int vcp_exclusive_scan_u32(vcp_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, int64_t n,
                           uint32_t* d_total);
int vcp_exclusive_max_scan_u32(vcp_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, int64_t n,
                           uint32_t* d_total);
