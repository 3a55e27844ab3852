// mugrid.hpp -- the uniform 3-D grid over the finite truths that vcp_match_unique (match_unique.hip) and
// vcp_register_pairs (register.hip) take their candidates from: cell edge h >= dist (1 + 2^-20), doubled until the grid has
// at most 2^22 cells, so a query meets every truth closer than dist in the 3 x 3 x 3 cells around its own.  dist = +inf, or
// an h that cannot be represented, is ONE cell: all truths, slow and correct.  Each translation unit gets its own copy of
// the two kernels and works in its own buffers.
#pragma once
#include <cmath>

#include "bounds.hpp"
#include "vcp_ctx.hpp"

namespace {
constexpr int MT = 128;
constexpr uint32_t NOCELL = 0xFFFFFFFFu;

// inv_h == 0: one cell (Dx = Dy = Dz = 1)
struct MUGrid {
  double x0, y0, z0, inv_h;
  int Dx, Dy, Dz;
};

// cell of every finite truth (NOCELL otherwise) and the population of every cell
__global__ __launch_bounds__(MT) void k_mu_cell(const double* __restrict__ truths, int T, MUGrid g,
                                                uint32_t* __restrict__ cellof, uint32_t* __restrict__ count) {
  const int i = (int)((int64_t)blockIdx.x * MT + threadIdx.x);
  if (i >= T) return;
  const double x = truths[3 * i], y = truths[3 * i + 1], z = truths[3 * i + 2];
  uint32_t c = NOCELL;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    c = 0u;
    if (g.inv_h != 0.0) {
      int cx = (int)floor((x - g.x0) * g.inv_h), cy = (int)floor((y - g.y0) * g.inv_h),
          cz = (int)floor((z - g.z0) * g.inv_h);
      cx = min(max(cx, 0), g.Dx - 1);
      cy = min(max(cy, 0), g.Dy - 1);
      cz = min(max(cz, 0), g.Dz - 1);
      c = (uint32_t)(((size_t)cz * g.Dy + cy) * g.Dx + cx);
    }
    atomicAdd(&count[c], 1u);
  }
  cellof[i] = c;
}

// the truths cell by cell: coordinates and original index (the order inside a cell is whatever the atomics give; every
// reader takes a minimum over the cell, or asks whether the cell holds some truth with a property)
__global__ __launch_bounds__(MT) void k_mu_fill(const double* __restrict__ truths, int T,
                                                const uint32_t* __restrict__ cellof,
                                                const uint32_t* __restrict__ cellstart, uint32_t* __restrict__ cur,
                                                double* __restrict__ sxyz, int32_t* __restrict__ sidx) {
  const int i = (int)((int64_t)blockIdx.x * MT + threadIdx.x);
  if (i >= T) return;
  const uint32_t c = cellof[i];
  if (c == NOCELL) return;
  const uint32_t s = cellstart[c] + atomicAdd(&cur[c], 1u);
  sxyz[3 * (size_t)s] = truths[3 * i];
  sxyz[3 * (size_t)s + 1] = truths[3 * i + 1];
  sxyz[3 * (size_t)s + 2] = truths[3 * i + 2];
  sidx[s] = i;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// cell edge >= max_dist (1 + 2^-20), doubled until the box of the finite truths has at most 2^22 cells; one cell when
// max_dist is infinite or no such edge (or its reciprocal) is a finite positive number
MUGrid plan_grid(const double lo[3], const double hi[3], double max_dist) {
  MUGrid g{lo[0], lo[1], lo[2], 0.0, 1, 1, 1};
  const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  double h = max_dist * (1.0 + 1.0 / 1048576.0);
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

// Where a build works: the caller's per-truth arrays, its bounds words ([d_box 64 bytes | d_part vcp_bounds_parts(T) * 64])
// and the buffer the cell starts go to.
struct MUGridWork {
  uint32_t* cellof;  // [T]
  double* sxyz;      // [T*3]
  int32_t* sidx;     // [T]
  double* d_box;
  double* d_part;
  DevBuf* b_cell;  // [cellstart (cells + 1) | cursors cells]
};

// Builds the grid of the T truths for max_dist on the context's stream (one synchronisation: the bounds, read back
// through ctx->pinned [0, 56)).  *have stays false -- no grid, nothing within max_dist of anything -- when max_dist is NaN
// or <= 0 or some axis has no finite value; a truth with a non-finite coordinate is in no cell.
int mu_build_grid(vcp_ctx* ctx, const double* d_truths, int T, double max_dist, const MUGridWork& w, MUGrid* g_out,
                  const uint32_t** cellstart_out, bool* have) {
  *have = false;
  if (!(max_dist > 0.0)) return VCP_OK;  // NaN or <= 0: no candidate at all
  hipStream_t st = ctx->stream;
  double* hb = reinterpret_cast<double*>(ctx->pinned);
  VCP_TRY(vcp_bounds(ctx, BoundsSrc{d_truths, T, 3, 3}, w.d_part, w.d_box, hb));
  const double lo[3] = {hb[0], hb[1], hb[2]}, hi[3] = {hb[3], hb[4], hb[5]};
  if (!(hi[0] >= lo[0] && hi[1] >= lo[1] && hi[2] >= lo[2])) return VCP_OK;  // an axis without a finite value
  const MUGrid g = plan_grid(lo, hi, max_dist);
  const size_t nc = (size_t)g.Dx * g.Dy * g.Dz;
  VCP_TRY(vcp_ensure(ctx, *w.b_cell, up16((nc + 1) * 4) + nc * 4));
  uint32_t* cellstart = w.b_cell->as<uint32_t>();
  uint32_t* cur = reinterpret_cast<uint32_t*>(w.b_cell->as<char>() + up16((nc + 1) * 4));
  VCP_HIP(ctx, hipMemsetAsync(cellstart, 0, up16((nc + 1) * 4) + nc * 4, st));
  VCP_LAUNCH(ctx, k_mu_cell, dim3(vcp_blocks(T, MT)), dim3(MT), 0, st, d_truths, T, g, w.cellof, cellstart);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, cellstart, cellstart, (int64_t)nc + 1, nullptr));
  VCP_LAUNCH(ctx, k_mu_fill, dim3(vcp_blocks(T, MT)), dim3(MT), 0, st, d_truths, T, w.cellof, cellstart, cur, w.sxyz,
             w.sidx);
  *g_out = g;
  *cellstart_out = cellstart;
  *have = true;  // (a finite value on every axis; a truth with all three finite may still be missing)
  return VCP_OK;
}
}  // namespace
