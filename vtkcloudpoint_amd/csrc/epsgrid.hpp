// epsgrid.hpp -- the uniform grid over the finite points that vcp_match_unique (match_unique.hip), vcp_register_pairs /
// vcp_register_sim (register.hip), vcp_eps_tree (eps_tree.hip) and vcp_gdbscan (gdbscan.hip) take their candidates from
// (DESIGN.md section 27).  Cell edge h >= d (1 + 2^-20), doubled until the box has at most 2^22 cells: every metric of
// these calls is >= each coordinate difference, so whatever lies within d of a point lies in the 3^dim cells around its
// own.  d = +inf, or an h that cannot be represented, is ONE cell: all points, slow and correct.  The points are binned
// into [cellstart (cells + 1) | cursors]; the order INSIDE a cell is whatever the atomics give, and every reader takes a
// minimum, a maximum, an integer sum or an existence over it.  Each translation unit gets its own copy of the kernels
// (anonymous namespace) and works in its own buffers.
#pragma once
#include <cmath>
#include <type_traits>

#include "bounds.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr uint32_t NOCELL = 0xFFFFFFFFu;
constexpr uint32_t HEAVY = 512;       // more points than this in a slot's 3^dim cells: the caller's heavy kernels
constexpr uint32_t DENSE_CHUNK = 16;  // a heavy chunk with fewer slots: one wave per slot

// inv_h == 0: one cell (Dx = Dy = Dz = 1)
struct EpsGrid {
  double x0, y0, z0, inv_h;
  int Dx, Dy, Dz;
};

// cell edge >= d (1 + 2^-20), doubled until the box has at most 2^22 cells; one cell when d is infinite, an extent is
// not finite or no such edge (or its reciprocal) is a finite positive number
EpsGrid eg_plan(const double lo[3], const double hi[3], double d) {
  EpsGrid g{lo[0], lo[1], lo[2], 0.0, 1, 1, 1};
  const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  double h = d * (1.0 + 1.0 / 1048576.0);
  if (!std::isfinite(h) || !(h > 0.0) || !std::isfinite(ex) || !std::isfinite(ey) || !std::isfinite(ez)) return g;
  for (int it = 0; it < 2200 && std::isfinite(h); it++, h *= 2.0) {
    const double dx = ex / h, dy = ey / h, dz = ez / h;
    if (!((dx + 1.0) * (dy + 1.0) * (dz + 1.0) <= 4194304.0)) continue;
    const double inv = 1.0 / h;
    if (!std::isfinite(inv) || !(inv > 0.0)) continue;
    g.inv_h = inv;
    g.Dx = (int)dx + 1;
    g.Dy = (int)dy + 1;
    g.Dz = (int)dz + 1;
    return g;
  }
  return g;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

__device__ __forceinline__ bool eg_finite(const double* q) { return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]); }

// the cell a finite point is binned into: clamped, so that a point on the box's upper faces is in the last cell
__device__ __forceinline__ void eg_cell_xyz(const EpsGrid& g, double x, double y, double z, int& cx, int& cy, int& cz) {
  cx = cy = cz = 0;
  if (g.inv_h == 0.0) return;
  cx = min(max((int)floor((x - g.x0) * g.inv_h), 0), g.Dx - 1);
  cy = min(max((int)floor((y - g.y0) * g.inv_h), 0), g.Dy - 1);
  cz = min(max((int)floor((z - g.z0) * g.inv_h), 0), g.Dz - 1);
}

__device__ __forceinline__ uint32_t eg_cell_of(const EpsGrid& g, double x, double y, double z) {
  int cx, cy, cz;
  eg_cell_xyz(g, x, y, z, cx, cy, cz);
  return (uint32_t)(((size_t)cz * g.Dy + cy) * g.Dx + cx);
}

// f(arguments); true when f returns true, which stops the loop that called it.  An f that returns nothing never stops.
template <class F, class... A>
__device__ __forceinline__ bool eg_stops(F&& f, const A&... a) {
  if constexpr (std::is_void_v<decltype(f(a...))>) {
    f(a...);
    return false;
  } else {
    return f(a...);
  }
}

// ---- row ranges -------------------------------------------------------------------------------------------------------
// f(first slot, one past the last) for every row of cells [xa, xb] x {y} x {z} of the block
template <class F>
__device__ __forceinline__ void eg_rows(const EpsGrid& g, const uint32_t* cellstart, int xa, int xb, int ya, int yb, int za,
                                        int zb, F&& f) {
  for (int z = za; z <= zb; z++)
    for (int y = ya; y <= yb; y++) {
      const size_t row = ((size_t)z * g.Dy + y) * g.Dx;
      if (eg_stops(f, cellstart[row + xa], cellstart[row + xb + 1])) return;
    }
}

// The rows of the 3^dim cells around a point that WAS binned: it is looked up in the cell it was binned into (clamped).
// Not the query form with a finite point: on the box's upper faces the two choose different cells, so the same
// neighbours in another order and another population count.
template <class F>
__device__ __forceinline__ void eg_member_rows(const EpsGrid& g, const uint32_t* cellstart, double x, double y, double z,
                                               F&& f) {
  int cx, cy, cz;
  eg_cell_xyz(g, x, y, z, cx, cy, cz);
  eg_rows(g, cellstart, max(cx - 1, 0), min(cx + 1, g.Dx - 1), max(cy - 1, 0), min(cy + 1, g.Dy - 1), max(cz - 1, 0),
          min(cz + 1, g.Dz - 1), f);
}

// The rows of the 3 x 3 x 3 cells around an arbitrary point m: none when m is NaN, more than one cell outside the box
// (nothing is within d of it) or, with one cell, not finite.
template <class F>
__device__ __forceinline__ void eg_query_rows(const EpsGrid& g, const uint32_t* cellstart, const double* m, F&& f) {
  int xa = 0, xb = 0, ya = 0, yb = 0, za = 0, zb = 0;
  if (g.inv_h == 0.0) {
    if (!eg_finite(m)) return;
  } else {
    const double ux = (m[0] - g.x0) * g.inv_h, uy = (m[1] - g.y0) * g.inv_h, uz = (m[2] - g.z0) * g.inv_h;
    if (!(ux >= -1.0 && ux < (double)g.Dx + 1.0 && uy >= -1.0 && uy < (double)g.Dy + 1.0 && uz >= -1.0 &&
          uz < (double)g.Dz + 1.0))
      return;
    const int cx = (int)floor(ux), cy = (int)floor(uy), cz = (int)floor(uz);
    xa = max(cx - 1, 0), xb = min(cx + 1, g.Dx - 1);
    ya = max(cy - 1, 0), yb = min(cy + 1, g.Dy - 1);
    za = max(cz - 1, 0), zb = min(cz + 1, g.Dz - 1);
    if (xa > xb) return;
  }
  eg_rows(g, cellstart, xa, xb, ya, yb, za, zb, f);
}

// ---- binning ----------------------------------------------------------------------------------------------------------
// A build reads its points and writes its records through a source type of the caller's:
//   void load(int64_t i, double q[3])                     the coordinates of point i (z = 0 in the plane)
//   bool in_grid(int64_t i, const double q[3])            whether point i is binned
//   void outside(int64_t i)                               what a point that is not binned gets
//   void store(uint32_t s, int64_t i, const double q[3])  the record of slot s, which point i takes
template <int GD>
__device__ __forceinline__ void load_pt(const double* __restrict__ c, int64_t i, int stride, double* q) {
#pragma unroll
  for (int a = 0; a < GD; a++) q[a] = c[i * stride + a];
  if (GD == 2) q[2] = 0.0;
}

// cell of every binned point (NOCELL otherwise) and the population of every cell
template <int WG, class Src>
__global__ __launch_bounds__(WG) void k_eg_cell(Src src, int64_t n, EpsGrid g, uint32_t* __restrict__ cellof,
                                                uint32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  double q[3];
  src.load(i, q);
  uint32_t cell = NOCELL;
  if (src.in_grid(i, q)) {
    cell = eg_cell_of(g, q[0], q[1], q[2]);
    atomicAdd(&count[cell], 1u);
  } else {
    src.outside(i);
  }
  cellof[i] = cell;
}

// the binned points cell by cell
template <int WG, class Src>
__global__ __launch_bounds__(WG) void k_eg_fill(Src src, int64_t n, const uint32_t* __restrict__ cellof,
                                                const uint32_t* __restrict__ cellstart, uint32_t* __restrict__ cur) {
  const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t cell = cellof[i];
  if (cell == NOCELL) return;
  const uint32_t s = cellstart[cell] + atomicAdd(&cur[cell], 1u);
  double q[3];
  src.load(i, q);
  src.store(s, i, q);
}

// Bins the n points of src by g on the context's stream, workgroups of WG: b_cell becomes [cellstart (cells + 1) | cursors
// cells], cleared, counted (k_eg_cell), scanned and filled (k_eg_fill).  cellof is the caller's, [n].
template <int WG, class Src>
int eg_bin(vcp_ctx* ctx, const Src& src, int64_t n, const EpsGrid& g, uint32_t* cellof, DevBuf& b_cell,
           const uint32_t** cellstart_out) {
  hipStream_t st = ctx->stream;
  const size_t nc = (size_t)g.Dx * g.Dy * g.Dz, o_cur = up16((nc + 1) * 4);
  VCP_TRY(vcp_ensure(ctx, b_cell, o_cur + nc * 4));
  uint32_t* cellstart = b_cell.as<uint32_t>();
  uint32_t* cur = reinterpret_cast<uint32_t*>(b_cell.as<char>() + o_cur);
  VCP_HIP(ctx, hipMemsetAsync(cellstart, 0, o_cur + nc * 4, st));
  VCP_LAUNCH(ctx, (k_eg_cell<WG, Src>), dim3(vcp_blocks(n, WG)), dim3(WG), 0, st, src, n, g, cellof, cellstart);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, cellstart, cellstart, (int64_t)nc + 1, nullptr));
  VCP_LAUNCH(ctx, (k_eg_fill<WG, Src>), dim3(vcp_blocks(n, WG)), dim3(WG), 0, st, src, n, cellof, cellstart, cur);
  *cellstart_out = cellstart;
  return VCP_OK;
}

// ---- the truths grid of vcp_match_unique and vcp_register_* -------------------------------------------------------------
// coordinates and original index of every truth with three finite coordinates; the others are in no cell
struct TruthSrc {
  const double* truths;
  double* sxyz;   // [T*3] cell order
  int32_t* sidx;  // [T]
  __device__ void load(int64_t i, double* q) const { load_pt<3>(truths, i, 3, q); }
  __device__ bool in_grid(int64_t, const double* q) const { return eg_finite(q); }
  __device__ void outside(int64_t) const {}
  __device__ void store(uint32_t s, int64_t i, const double* q) const {
    sxyz[3 * (size_t)s] = q[0];
    sxyz[3 * (size_t)s + 1] = q[1];
    sxyz[3 * (size_t)s + 2] = q[2];
    sidx[s] = (int32_t)i;
  }
};

// Where a build works: the caller's per-truth arrays, its bounds words ([d_box 64 bytes | d_part vcp_bounds_parts(T) * 64])
// and the buffer the cell starts go to.
struct TruthGridWork {
  uint32_t* cellof;  // [T]
  double* sxyz;      // [T*3]
  int32_t* sidx;     // [T]
  double* d_box;
  double* d_part;
  DevBuf* b_cell;
};

// Builds the grid of the T truths for max_dist on the context's stream, workgroups of WG (one synchronisation: the bounds,
// read back through ctx->pinned [0, 56)).  *have stays false -- no grid, nothing within max_dist of anything -- when max_dist is NaN
// or <= 0 or some axis has no finite value; a truth with a non-finite coordinate is in no cell.
template <int WG>
int eg_build_truths(vcp_ctx* ctx, const double* d_truths, int T, double max_dist, const TruthGridWork& w, EpsGrid* g_out,
                    const uint32_t** cellstart_out, bool* have) {
  *have = false;
  if (!(max_dist > 0.0)) return VCP_OK;  // NaN or <= 0: no candidate at all
  double* hb = reinterpret_cast<double*>(ctx->pinned);
  VCP_TRY(vcp_bounds(ctx, BoundsSrc{d_truths, T, 3, 3}, w.d_part, w.d_box, hb));
  const double lo[3] = {hb[0], hb[1], hb[2]}, hi[3] = {hb[3], hb[4], hb[5]};
  if (!(hi[0] >= lo[0] && hi[1] >= lo[1] && hi[2] >= lo[2])) return VCP_OK;  // an axis without a finite value
  *g_out = eg_plan(lo, hi, max_dist);
  VCP_TRY(eg_bin<WG>(ctx, TruthSrc{d_truths, w.sxyz, w.sidx}, T, *g_out, w.cellof, *w.b_cell, cellstart_out));
  *have = true;  // (a finite value on every axis; a truth with all three finite may still be missing)
  return VCP_OK;
}

// ---- records, the walk and the heavy chunks (vcp_eps_tree, vcp_gdbscan) -------------------------------------------------
// What a walk reads; the callers' argument structs begin with it.  A record is (x, y, z or 0, the caller's fourth word).
struct EpsCells {
  EpsGrid g;
  const uint32_t* cellstart;  // [cells + 1]; the last entry is the number of slots
  const double4* rec;         // [slots] cell order
};

// the distance expression of vcp_kdist / vcp_dbscan (binary64, left to right, -ffp-contract=off)
template <int METRIC>
__device__ __forceinline__ double dist(const double4& q, const double4& r) {
  const double dx = q.x - r.x, dy = q.y - r.y;
  if (METRIC == VCP_L1_2D) return fabs(dx) + fabs(dy);
  if (METRIC == VCP_L2_2D) return sqrt(dx * dx + dy * dy);
  const double dz = q.z - r.z;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// The candidates of the record q, four at a time so that their loads are in flight together: use(t, record) for every
// slot t of the rows that want(t) accepts, until a use returns true; lane `off` of `step` takes every step-th candidate.
template <class Want, class Use>
__device__ __forceinline__ void eg_walk(const EpsCells& c, const double4& q, uint32_t off, uint32_t step, Want&& want,
                                        Use&& use) {
  bool stop = false;
  eg_member_rows(c.g, c.cellstart, q.x, q.y, q.z, [&](uint32_t s0, uint32_t s1) {
    for (uint32_t t = s0 + off; t < s1 && !stop; t += 4u * step) {
      double4 r[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t tu = t + (uint32_t)u * step;
        ok[u] = tu < s1 && want(tu);
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (ok[u]) r[u] = c.rec[t + (uint32_t)u * step];
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (ok[u] && !stop) stop = eg_stops(use, t + (uint32_t)u * step, r[u]);
    }
  });
}

// more than HEAVY points in the 3^dim cells around the record q: the same for every slot of a cell
__device__ __forceinline__ bool eg_heavy_cell(const EpsCells& c, const double4& q) {
  uint32_t total = 0;
  eg_member_rows(c.g, c.cellstart, q.x, q.y, q.z, [&](uint32_t s0, uint32_t s1) { total += s1 - s0; });
  return total > HEAVY;
}

// The slots of a heavy cell go to the heavy kernels in chunks of <= 64 consecutive slots: whether slot s, of record q,
// begins a chunk of its cell
__device__ __forceinline__ bool eg_chunk_first(const EpsCells& c, const double4& q, uint32_t s) {
  return ((s - c.cellstart[eg_cell_of(c.g, q.x, q.y, q.z)]) & 63u) == 0;
}

// The list of heavy chunks: every lane of a wave calls this, with first = "my slot s begins a chunk of a heavy cell"; those
// slots are appended to list[] and counted in *count.
__device__ __forceinline__ void eg_list_chunks(bool first, uint32_t s, uint32_t* list, uint32_t* count) {
  const uint32_t slot = wave_append(first, count);
  if (first) list[slot] = s;
}

// one past the last slot of the chunk that starts at slot s0
__device__ __forceinline__ uint32_t eg_chunk_end(const EpsCells& c, uint32_t s0) {
  const double4 q = c.rec[s0];
  return min(s0 + 64u, c.cellstart[eg_cell_of(c.g, q.x, q.y, q.z) + 1u]);
}

// One wave (a workgroup of 64) per heavy chunk.  The slots of a chunk share their cell and so their candidate rows: with a
// lane per slot the wave walks the rows in step and every load serves all its lanes (per_lane(slot)).  A chunk of only a
// few slots (a sparse cell beside a dense one) would leave most lanes idle on a long walk: there the whole wave takes one
// slot at a time, the candidates dealt over the lanes (per_wave(slot, lane); wave-uniform).
template <class PerLane, class PerWave>
__device__ __forceinline__ void eg_heavy(const EpsCells& c, const uint32_t* list, uint32_t nheavy, PerLane&& per_lane,
                                         PerWave&& per_wave) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t h = blockIdx.x; h < nheavy; h += gridDim.x) {
    const uint32_t s0 = list[h], s1 = eg_chunk_end(c, s0);
    if (s1 - s0 >= DENSE_CHUNK) {
      if (s0 + lane < s1) per_lane(s0 + lane);
      continue;
    }
    for (uint32_t s = s0; s < s1; s++) per_wave(s, lane);
  }
}
}  // namespace
