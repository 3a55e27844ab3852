// bounds.hip -- bounding box (two launches: per-workgroup partials, one-workgroup fold) and the trimmed moments of the
// robust range (bounds.hpp).
#include <cmath>
#include <vector>

#include "bounds.hpp"
#include "grid_common.hpp"
#include "reduce.hpp"

using vcpg::load_in;

namespace {
constexpr int BT = 256;

template <int GD, bool GROUPED>
__global__ __launch_bounds__(BT) void k_bounds(const double* __restrict__ c, int64_t n, int stride,
                                              const int32_t* __restrict__ group, int glo, int ghi,
                                              double* __restrict__ part) {
  double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (int64_t)gridDim.x * BT) {
    if (GROUPED) {
      const int g = group[i];
      if (g < glo || g >= ghi) continue;
    }
    double q[3];
    load_in<GD>(c, i, stride, q);  // (one 16-byte load per point where the layout allows: 68 -> 40 us at 10 M points)
    bool bad = false;
#pragma unroll
    for (int a = 0; a < GD; a++) {
      if (isfinite(q[a])) {
        v[a] = fmin(v[a], q[a]);
        v[3 + a] = fmax(v[3 + a], q[a]);
      } else {
        bad = true;
      }
    }
    if (bad) v[6] += 1.0;
  }
  block_fold<BT>(v, FoldBox(), part + (size_t)blockIdx.x * 8);
}

__global__ __launch_bounds__(BT) void k_bounds_final(const double* __restrict__ part, int nb, double* __restrict__ out) {
  double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
  for (int b = threadIdx.x; b < nb; b += BT) {
#pragma unroll
    for (int a = 0; a < 7; a++) v[a] = FoldBox::op(a, v[a], part[(size_t)b * 8 + a]);
  }
  block_fold<BT>(v, FoldBox(), out);
}

// per axis the count, sum and sum of squares (about mid[a]) of the finite values inside [lo[a], hi[a]]:
// part[b*9 + 3a + {0,1,2}]
struct Range3 {
  double lo[3], hi[3], mid[3];
};
template <int GD, bool GROUPED>
__global__ __launch_bounds__(BT) void k_moments(const double* __restrict__ c, int64_t n, int stride,
                                               const int32_t* __restrict__ group, int glo, int ghi, Range3 R,
                                               double* __restrict__ part) {
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (int64_t)gridDim.x * BT) {
    if (GROUPED) {
      const int g = group[i];
      if (g < glo || g >= ghi) continue;
    }
#pragma unroll
    for (int a = 0; a < GD; a++) {
      const double v = c[i * stride + a];
      if (v >= R.lo[a] && v <= R.hi[a]) {
        const double d = v - R.mid[a];
        m[3 * a] += 1.0;
        m[3 * a + 1] += d;
        m[3 * a + 2] += d * d;
      }
    }
  }
  block_fold<BT>(m, FoldSum(), part + (size_t)blockIdx.x * 9);
}

template <int GD, bool GROUPED>
int launch_bounds(vcp_ctx* ctx, const BoundsSrc& s, int rb, hipStream_t st, double* d_part) {
  VCP_LAUNCH(ctx, (k_bounds<GD, GROUPED>), dim3(rb), dim3(BT), 0, st, s.c, s.n, s.stride, s.group, s.glo, s.ghi, d_part);
  return VCP_OK;
}
template <int GD, bool GROUPED>
int launch_moments(vcp_ctx* ctx, const BoundsSrc& s, int rb, hipStream_t st, const Range3& R, double* d_part) {
  VCP_LAUNCH(ctx, (k_moments<GD, GROUPED>), dim3(rb), dim3(BT), 0, st, s.c, s.n, s.stride, s.group, s.glo, s.ghi, R,
                  d_part);
  return VCP_OK;
}
}  // namespace

int vcp_bounds_parts(int64_t n) { return (int)vcp_blocks(n, BT, 1024); }

int vcp_bounds_dev(vcp_ctx* ctx, const BoundsSrc& s, double* d_part, double* d_out) {
  const int rb = vcp_bounds_parts(s.n);
  hipStream_t st = ctx->stream;
  if (s.gd == 2) {
    if (s.group) VCP_TRY((launch_bounds<2, true>(ctx, s, rb, st, d_part)));
    else VCP_TRY((launch_bounds<2, false>(ctx, s, rb, st, d_part)));
  } else {
    if (s.group) VCP_TRY((launch_bounds<3, true>(ctx, s, rb, st, d_part)));
    else VCP_TRY((launch_bounds<3, false>(ctx, s, rb, st, d_part)));
  }
  VCP_LAUNCH(ctx, k_bounds_final, dim3(1), dim3(BT), 0, st, d_part, rb, d_out);
  return VCP_OK;
}

int vcp_bounds(vcp_ctx* ctx, const BoundsSrc& s, double* d_part, double* d_out, double* h) {
  VCP_TRY(vcp_bounds_dev(ctx, s, d_part, d_out));
  VCP_HIP(ctx, hipMemcpyAsync(h, d_out, 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_robust_range(vcp_ctx* ctx, const BoundsSrc& s, DevBuf& part, double* lo, double* hi,
                     const std::function<double(double lo, double hi)>& pad,
                     const std::function<bool(const double* lo, const double* hi)>& done) {
  hipStream_t st = ctx->stream;
  const int rb = vcp_bounds_parts(s.n);
  std::vector<double> hm;
  for (int it = 0; it < 8 && !done(lo, hi); it++) {
    VCP_TRY(vcp_ensure(ctx, part, (size_t)rb * 9 * sizeof(double)));  // (only when a round runs: no workspace otherwise)
    double* d_mom = part.as<double>();
    hm.resize((size_t)rb * 9);
    Range3 R;
    for (int a = 0; a < 3; a++) {
      R.lo[a] = lo[a];
      R.hi[a] = hi[a];
      R.mid[a] = 0.5 * lo[a] + 0.5 * hi[a];
    }
    if (s.gd == 2) {
      if (s.group) VCP_TRY((launch_moments<2, true>(ctx, s, rb, st, R, d_mom)));
      else VCP_TRY((launch_moments<2, false>(ctx, s, rb, st, R, d_mom)));
    } else {
      if (s.group) VCP_TRY((launch_moments<3, true>(ctx, s, rb, st, R, d_mom)));
      else VCP_TRY((launch_moments<3, false>(ctx, s, rb, st, R, d_mom)));
    }
    VCP_HIP(ctx, hipMemcpyAsync(hm.data(), d_mom, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    bool changed = false;
    for (int a = 0; a < s.gd; a++) {
      double cnt = 0, s1 = 0, s2 = 0;
      for (int b = 0; b < rb; b++) {
        cnt += hm[(size_t)b * 9 + 3 * a];
        s1 += hm[(size_t)b * 9 + 3 * a + 1];
        s2 += hm[(size_t)b * 9 + 3 * a + 2];
      }
      if (!(cnt > 0)) continue;
      const double mean = s1 / cnt, var = std::fmax(s2 / cnt - mean * mean, 0.0);
      const double c0 = R.mid[a] + mean, w = 8.0 * std::sqrt(var) + pad(lo[a], hi[a]);
      const double nlo = std::fmax(lo[a], c0 - w), nhi = std::fmin(hi[a], c0 + w);
      if (nlo <= nhi && (nlo > lo[a] || nhi < hi[a])) {
        lo[a] = nlo;
        hi[a] = nhi;
        changed = true;
      }
    }
    if (!changed) break;
  }
  return VCP_OK;
}
