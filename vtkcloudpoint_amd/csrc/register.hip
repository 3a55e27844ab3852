// register.hip -- vcp_register_pairs: global registration of a centroid list to the truths by congruent pairs
// (include/vcp.h).  No start pose: a base (two source points) laid on an ordered pair of targets of
// the same length, within len_tol, is a planar rigid motion; every such motion is scored by the landmarks it puts within
// inlier_dist of some target, and the best one per base is kept.
//
//   k_regp_bases   per base: u = b' - a, Lu, the midpoint; an index outside the source raises the error word
//   (host)         the bases with 0 < Lu < inf sorted by Lu: sL (lengths) and sb (base of every sorted place)
//   k_regp_search  one workgroup per target i.  Its lanes stride over j and take Lv of (i, j) once; the bases whose length
//                  fits are a run of sL (fl(Lv - Lu) falls as Lu rises), found by binary search in LDS and walked with
//                  the header's exact test.  Every (place, f, j) that passes goes to an LDS queue, one slot count per
//                  wave; when the queue cannot take another round of pushes, and at the end of the row, the workgroup
//                  scores it: one wave per hypothesis, lanes over the landmarks, a ballot and a popcount per 64, then
//                  ONE 64-bit atomicMax on the base's word
//                      score << 33  |  (2^33 - 1 - (f << 32 | i << 16 | j))
//                  whose maximum is the highest score and, among equals, the lowest (f, i, j): nt <= 65 536 and
//                  score < 2^31 make the three fields fit, and i != j keeps every word above 0, which means "none".
//                  There is no global list of hypotheses and no second sweep for the tie.
//   k_regp_final   per base: the winner's word back to (score, f, i, j), M rebuilt from them by the same function, and the
//                  inliers over all ns source points
// The score is an existence test over the 3 x 3 x 3 cells of epsgrid.hpp's grid over the targets for inlier_dist.  Only
// integer atomics decide anything: the result does not depend on scheduling.
//
// vcp_register_sim is the same call with a scale: a base fits a target pair when k = Lv / Lu lies in
// [scale_min, scale_max], and the pose carries k (rg_sim_pose_of).  The search and the final kernel are one source for both
// (rg_search<SIM>, rg_final<SIM>); what differs is the length test, the pose function and the scale that is written:
//   k_regs_search  fl(Lv / Lu) does not rise as Lu rises (a correctly rounded division is monotone), so the passing bases
//                  are again one run of sL: its start by binary search on Lv / sL[mid] <= scale_max, then walked while
//                  Lv / sL[k] >= scale_min.  The exact division decides every place; there is no cheaper bracket
//   k_regs_final   k_regp_final with the similarity pose; also writes the winner's k
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "epsgrid.hpp"
#include "match.hpp"
#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int RT = 256;          // threads of a search / final workgroup
constexpr int RG_GRID_WG = 128;  // threads of a workgroup of the target grid's build
constexpr int RG_QCAP = 2 * RT;  // hypotheses the LDS queue holds: it is scored once it holds more than RG_QCAP - RT, and a
                                 // round of pushes adds at most RT
constexpr int RG_MAX_BASES = 4096;
constexpr int RG_MAX_TARGETS = 65536;
constexpr unsigned long long RG_LOW = (1ull << 33) - 1ull;

struct RGScan {
  EpsGrid g;
  const uint32_t* cellstart;  // nullptr: no grid, nothing is within inlier_dist of anything
  const double* sxyz;
  double inlier_dist;
};

// the base table: six arrays of `stride` doubles
struct RGTab {
  const double* t;
  int stride;
  __device__ double Lu(int b) const { return t[b]; }
  __device__ double ux(int b) const { return t[(size_t)stride + b]; }
  __device__ double uy(int b) const { return t[2 * (size_t)stride + b]; }
  __device__ double msx(int b) const { return t[3 * (size_t)stride + b]; }
  __device__ double msy(int b) const { return t[4 * (size_t)stride + b]; }
  __device__ double msz(int b) const { return t[5 * (size_t)stride + b]; }
};

// The record of a base (a, b'): r = (Lu, ux, uy, ms.x, ms.y, ms.z), vcp.h's expressions.  Host and device run this source.
__host__ __device__ inline void rg_base(const double* a, const double* b, double r[6]) {
  const double ux = b[0] - a[0], uy = b[1] - a[1];
  r[0] = sqrt(ux * ux + uy * uy);
  r[1] = ux;
  r[2] = uy;
  r[3] = (a[0] + b[0]) * 0.5;
  r[4] = (a[1] + b[1]) * 0.5;
  r[5] = (a[2] + b[2]) * 0.5;
}

// The pose of a hypothesis from its base's record r, the flip f and the two targets: vcp.h's formulas in their operand
// order; false when the hypothesis is skipped (nrm).  Host and device run this source.
__host__ __device__ inline bool rg_pose_of(const double r[6], int f, const double* ti, const double* tj, double M[16]) {
  double ux = r[1], uy = r[2], msx = r[3], msy = r[4];
  const double msz = r[5];
  if (f) {  // the source read as (x, -y, z): both the difference and the midpoint change sign exactly
    uy = -uy;
    msy = -msy;
  }
  const double ix = ti[0], iy = ti[1], iz = ti[2], jx = tj[0], jy = tj[1], jz = tj[2];
  const double vx = jx - ix, vy = jy - iy;
  const double dot = ux * vx + uy * vy, crs = ux * vy - uy * vx;
  const double nrm = sqrt(dot * dot + crs * crs);
  if (!(nrm > 0.0 && nrm < INFINITY)) return false;
  const double c = dot / nrm, s = crs / nrm;
  const double mtx = (ix + jx) * 0.5, mty = (iy + jy) * 0.5, mtz = (iz + jz) * 0.5;
  M[0] = c;
  M[1] = f ? s : -s;
  M[2] = 0.0;
  M[3] = mtx - (c * msx - s * msy);
  M[4] = s;
  M[5] = f ? -c : c;
  M[6] = 0.0;
  M[7] = mty - (s * msx + c * msy);
  M[8] = 0.0;
  M[9] = 0.0;
  M[10] = 1.0;
  M[11] = mtz - msz;
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
  return true;
}

// The similarity pose: rg_pose_of's rotation and midpoints with k = Lv / Lu on the rotation block and on the moved source
// midpoint; *scale = k.  False when the hypothesis is skipped (nrm).  With k == 1.0 every entry of M is rg_pose_of's bit for
// bit (1.0 * x == x, sign of zero included).  Host and device run this source.
__host__ __device__ inline bool rg_sim_pose_of(const double r[6], int f, const double* ti, const double* tj, double M[16],
                                               double* scale) {
  double ux = r[1], uy = r[2], msx = r[3], msy = r[4];
  const double msz = r[5];
  if (f) {
    uy = -uy;
    msy = -msy;
  }
  const double ix = ti[0], iy = ti[1], iz = ti[2], jx = tj[0], jy = tj[1], jz = tj[2];
  const double vx = jx - ix, vy = jy - iy;
  const double k = sqrt(vx * vx + vy * vy) / r[0];
  *scale = k;
  const double dot = ux * vx + uy * vy, crs = ux * vy - uy * vx;
  const double nrm = sqrt(dot * dot + crs * crs);
  if (!(nrm > 0.0 && nrm < INFINITY)) return false;
  const double c = dot / nrm, s = crs / nrm;
  const double kc = k * c, ks = k * s;
  const double mtx = (ix + jx) * 0.5, mty = (iy + jy) * 0.5, mtz = (iz + jz) * 0.5;
  M[0] = kc;
  M[1] = f ? ks : -ks;
  M[2] = 0.0;
  M[3] = mtx - (kc * msx - ks * msy);
  M[4] = ks;
  M[5] = f ? -kc : kc;
  M[6] = 0.0;
  M[7] = mty - (ks * msx + kc * msy);
  M[8] = 0.0;
  M[9] = 0.0;
  M[10] = k;
  M[11] = mtz - k * msz;
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
  return true;
}

__global__ __launch_bounds__(RT) void k_regp_bases(const double* __restrict__ src, int64_t ns,
                                                   const int32_t* __restrict__ bases, int nb, double* __restrict__ tab,
                                                   uint32_t* __restrict__ err) {
  const int b = (int)(blockIdx.x * RT + threadIdx.x);
  if (b >= nb) return;
  const int64_t a = bases[2 * b], c = bases[2 * b + 1];
  if (a < 0 || a >= ns || c < 0 || c >= ns) {
    atomicOr(err, 1u);
    return;
  }
  double r[6];
  rg_base(src + 3 * a, src + 3 * c, r);
#pragma unroll
  for (int t = 0; t < 6; t++) tab[(size_t)t * nb + b] = r[t];
}

// does some target lie closer than inlier_dist to m?  vcp_match's distance, strict comparison
__device__ __forceinline__ bool rg_exists(const RGScan& q, const double* m) {
  if (!q.cellstart) return false;
  bool found = false;
  eg_query_rows(q.g, q.cellstart, m, [&](uint32_t s0, uint32_t s1) {
    for (uint32_t s = s0; s < s1; s++) {
      const double dx = q.sxyz[3 * (size_t)s] - m[0], dy = q.sxyz[3 * (size_t)s + 1] - m[1],
                   dz = q.sxyz[3 * (size_t)s + 2] - m[2];
      if (sqrt(dx * dx + dy * dy + dz * dz) < q.inlier_dist) return found = true;
    }
    return false;
  });
  return found;
}

// The pose of hypothesis (b, f, i, j) from the base table; SIM: the similarity pose and its scale.
template <bool SIM>
__device__ __forceinline__ bool rg_pose(const RGTab& tab, int b, int f, const double* __restrict__ tgt, int i, int j,
                                        double M[16], double* scale) {
  const double r[6] = {tab.Lu(b), tab.ux(b), tab.uy(b), tab.msx(b), tab.msy(b), tab.msz(b)};
  if (SIM) return rg_sim_pose_of(r, f, tgt + 3 * (size_t)i, tgt + 3 * (size_t)j, M, scale);
  return rg_pose_of(r, f, tgt + 3 * (size_t)i, tgt + 3 * (size_t)j, M);
}

struct RGSearch {
  const double* src;  // landmark l is source point l * step
  int64_t step;
  int nl;
  const double* tgt;
  int nt;
  RGTab tab;
  const double* sL;   // [nv] ascending
  const int32_t* sb;  // [nv] base of the sorted place
  int nv;
  double len_tol;               // the rigid search
  double scale_min, scale_max;  // the similarity search
  int nf;                       // 1, or 2 with the mirror images
  RGScan q;
  unsigned long long* key;   // [n_bases] the winners' words
  unsigned long long* nhyp;  // [n_bases]
};

// scores the n queued hypotheses of row i: wave w takes entries w, w + 4, ...
template <bool SIM>
__device__ __forceinline__ void rg_flush(const RGSearch& a, int i, const uint32_t* qe, uint32_t n) {
  const int lane = threadIdx.x & 63;
  for (uint32_t e = threadIdx.x >> 6; e < n; e += RT / 64) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)qe[e]);
    const int j = (int)(w & 0xFFFFu), f = (int)((w >> 16) & 1u), b = a.sb[w >> 17];
    double M[16], sc;
    const bool ok = rg_pose<SIM>(a.tab, b, f, a.tgt, i, j, M, &sc);
    uint32_t cnt = 0;
    if (ok) {
      for (int l0 = 0; l0 < a.nl; l0 += 64) {
        const int l = l0 + lane;
        bool hit = false;
        if (l < a.nl) {
          const double* p = a.src + 3 * (size_t)l * (size_t)a.step;
          double m[3];
          mtc::transform(M, p[0], p[1], p[2], m);
          hit = rg_exists(a.q, m);
        }
        cnt += wave_count(hit);
      }
    }
    if (lane == 0) {
      atomicAdd(&a.nhyp[b], 1ull);
      if (ok) {
        const unsigned long long pk = ((unsigned long long)f << 32) | ((unsigned long long)i << 16) | (unsigned long long)j;
        const unsigned long long k = ((unsigned long long)cnt << 33) | (RG_LOW - pk);
        if (k > __hip_atomic_load(&a.key[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a.key[b], k);
      }
    }
  }
}

// does the base at sorted place k fit a target pair of length Lv?  The header's test, on the operands it names.
template <bool SIM>
__device__ __forceinline__ bool rg_fits(const RGSearch& a, double Lv, const double* sL, int k) {
  if (k >= a.nv) return false;
  if (SIM) {
    const double r = Lv / sL[k];
    return a.scale_min <= r && r <= a.scale_max;
  }
  return fabs(Lv - sL[k]) <= a.len_tol;
}

// The search of one workgroup (target i = blockIdx.x); sL, qe and qn are the kernel's LDS.
template <bool SIM>
__device__ __forceinline__ void rg_search(const RGSearch& a, double* sL, uint32_t* qe, uint32_t* qn) {
  const int tid = threadIdx.x;
  for (int k = tid; k < a.nv; k += RT) sL[k] = a.sL[k];
  if (tid == 0) *qn = 0;
  __syncthreads();
  const int i = blockIdx.x;
  const double ix = a.tgt[3 * (size_t)i], iy = a.tgt[3 * (size_t)i + 1];
  for (int j0 = 0; j0 < a.nt; j0 += RT) {
    const int j = j0 + tid;
    int k = 0, f = 0;
    double Lv = 0.0;
    bool live = false;
    if (j < a.nt && j != i) {
      const double vx = a.tgt[3 * (size_t)j] - ix, vy = a.tgt[3 * (size_t)j + 1] - iy;
      Lv = sqrt(vx * vx + vy * vy);
      if (Lv > 0.0 && Lv < INFINITY) {
        // the first place with fl(Lv - Lu) <= len_tol (SIM: fl(Lv / Lu) <= scale_max); both fall as Lu rises
        int lo = 0, hi = a.nv;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (SIM ? Lv / sL[mid] <= a.scale_max : Lv - sL[mid] <= a.len_tol)
            hi = mid;
          else
            lo = mid + 1;
        }
        k = lo;
        live = rg_fits<SIM>(a, Lv, sL, k);
      }
    }
    // a round: every lane that still has a hypothesis queues one; the queue is scored when the next round might not fit
    while (__syncthreads_or(live)) {
      const uint32_t slot = wave_append(live, qn);
      if (live) qe[slot] = (uint32_t)j | ((uint32_t)f << 16) | ((uint32_t)k << 17);
      if (live && ++f == a.nf) {
        f = 0;
        k++;
        live = rg_fits<SIM>(a, Lv, sL, k);
      }
      __syncthreads();
      const uint32_t n = *qn;
      if (n > RG_QCAP - RT) {  // workgroup-uniform
        rg_flush<SIM>(a, i, qe, n);
        __syncthreads();
        if (tid == 0) *qn = 0;
      }
    }
  }
  rg_flush<SIM>(a, i, qe, *qn);
}

__global__ __launch_bounds__(RT) void k_regp_search(RGSearch a) {
  __shared__ double sL[RG_MAX_BASES];
  __shared__ uint32_t qe[RG_QCAP];
  __shared__ uint32_t qn;
  rg_search<false>(a, sL, qe, &qn);
}

__global__ __launch_bounds__(RT) void k_regs_search(RGSearch a) {
  __shared__ double sL[RG_MAX_BASES];
  __shared__ uint32_t qe[RG_QCAP];
  __shared__ uint32_t qn;
  rg_search<true>(a, sL, qe, &qn);
}

// grid (source points, bases)
template <bool SIM>
__device__ __forceinline__ void rg_final(const double* __restrict__ src, int64_t ns, const double* __restrict__ tgt,
                                         const RGTab& tab, const unsigned long long* __restrict__ key, const RGScan& q,
                                         double* __restrict__ M_all, int32_t* __restrict__ score, int32_t* __restrict__ pick,
                                         uint32_t* __restrict__ inliers, double* __restrict__ scale, double* sM, int* has,
                                         uint32_t* wc) {
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    const unsigned long long k = key[b];
    double M[16], kw = 0.0;  // the winner's scale
    int sc = -1, f = 0, i = -1, j = -1;
    bool ok = false;
    if (k != 0ull) {
      const unsigned long long pk = RG_LOW - (k & RG_LOW);
      sc = (int)(k >> 33);
      f = (int)(pk >> 32);
      i = (int)((pk >> 16) & 0xFFFFull);
      j = (int)(pk & 0xFFFFull);
      ok = rg_pose<SIM>(tab, b, f, tgt, i, j, M, &kw);  // true: the word came from a pose that was scored
    }
    if (!ok) {
      sc = -1, f = 0, i = -1, j = -1;
      kw = 0.0;
      for (int t = 0; t < 16; t++) M[t] = 0.0;
    }
    for (int t = 0; t < 16; t++) sM[t] = M[t];
    *has = ok;
    if (blockIdx.x == 0) {
      for (int t = 0; t < 16; t++) M_all[16 * (size_t)b + t] = M[t];
      score[b] = sc;
      pick[3 * b] = f;
      pick[3 * b + 1] = i;
      pick[3 * b + 2] = j;
      if (SIM) scale[b] = kw;
    }
  }
  __syncthreads();
  if (!*has) return;
  const int64_t p = (int64_t)blockIdx.x * RT + threadIdx.x;
  bool hit = false;
  if (p < ns) {
    double M[16], m[3];
#pragma unroll
    for (int t = 0; t < 16; t++) M[t] = sM[t];
    mtc::transform(M, src[3 * p], src[3 * p + 1], src[3 * p + 2], m);
    hit = rg_exists(q, m);
  }
  uint32_t t;
  if (block_count<RT>(hit, wc, t) && t) atomicAdd(&inliers[b], t);
}

__global__ __launch_bounds__(RT) void k_regp_final(const double* __restrict__ src, int64_t ns,
                                                   const double* __restrict__ tgt, RGTab tab,
                                                   const unsigned long long* __restrict__ key, RGScan q,
                                                   double* __restrict__ M_all, int32_t* __restrict__ score,
                                                   int32_t* __restrict__ pick, uint32_t* __restrict__ inliers) {
  __shared__ double sM[16];
  __shared__ int has;
  __shared__ uint32_t wc[RT / 64];
  rg_final<false>(src, ns, tgt, tab, key, q, M_all, score, pick, inliers, nullptr, sM, &has, wc);
}

__global__ __launch_bounds__(RT) void k_regs_final(const double* __restrict__ src, int64_t ns,
                                                   const double* __restrict__ tgt, RGTab tab,
                                                   const unsigned long long* __restrict__ key, RGScan q,
                                                   double* __restrict__ M_all, int32_t* __restrict__ score,
                                                   int32_t* __restrict__ pick, uint32_t* __restrict__ inliers,
                                                   double* __restrict__ scale) {
  __shared__ double sM[16];
  __shared__ int has;
  __shared__ uint32_t wc[RT / 64];
  rg_final<true>(src, ns, tgt, tab, key, q, M_all, score, pick, inliers, scale, sM, &has, wc);
}

// what a target pair must satisfy to fit a base: |Lv - Lu| <= len_tol, or (sim) scale_min <= Lv / Lu <= scale_max
struct RGFit {
  bool sim;
  double len_tol, scale_min, scale_max;
};

int rg_check(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, const int32_t* bases,
             int32_t n_bases, const RGFit& fit, int max_landmarks, double inlier_dist, const double* M_best,
             const int32_t* best) {
  if (!source || !target || !bases || !M_best || !best) return vcp_fail(ctx, VCP_ERR_ARG, "null argument");
  if (n_bases < 1) return vcp_fail(ctx, VCP_ERR_ARG, "n_bases < 1");
  if (max_landmarks < 1) return vcp_fail(ctx, VCP_ERR_ARG, "max_landmarks < 1");
  if (fit.sim) {
    if (!(fit.scale_min > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "scale_min must be > 0");
    if (!(fit.scale_max >= fit.scale_min && fit.scale_max < INFINITY))
      return vcp_fail(ctx, VCP_ERR_ARG, "scale_max must be finite and >= scale_min");
  } else if (!(fit.len_tol >= 0.0)) {
    return vcp_fail(ctx, VCP_ERR_ARG, "len_tol must be >= 0 (+inf allowed)");
  }
  if (!(inlier_dist > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "inlier_dist must be > 0 (+inf allowed)");
  if (ns < 2 || nt < 2) return vcp_fail(ctx, VCP_ERR_EMPTY, "fewer than two source or target points");
  if (n_bases > RG_MAX_BASES) return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "n_bases > %d", RG_MAX_BASES);
  if (nt > RG_MAX_TARGETS)
    return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "nt > %d (the pair enumeration is quadratic in nt)", RG_MAX_TARGETS);
  if (ns > 0x7FFFFFFFLL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "ns beyond 32-bit indexing");
  return VCP_OK;
}

// the per-base results as they lie in b_rg_work and, read back, in the pinned stage
struct RGLayout {
  size_t o_M, o_nhyp, o_score, o_inl, o_pick, o_scale, bytes;
  explicit RGLayout(size_t nb, bool sim = false) {
    o_M = 0;
    o_nhyp = o_M + nb * 128;
    o_score = o_nhyp + nb * 8;
    o_inl = o_score + nb * 4;
    o_pick = o_inl + nb * 4;
    o_scale = bytes = up16(o_pick + nb * 12);
    if (sim) bytes = up16(o_scale + nb * 8);  // the winners' scales, vcp_register_sim only
  }
};

// The call on device pointers.  The per-base results stay in b_rg_work (at *res_dev) and are read back to *res_host,
// laid out by RGLayout; M_best and best are filled.
int rg_run(vcp_ctx* ctx, const double* d_src, int64_t ns, const double* d_tgt, int64_t nt, const int32_t* d_bases,
           int32_t n_bases, const RGFit& fit, int mirror, int max_landmarks, double inlier_dist, double M_best[16],
           int32_t* best, const char** res_dev, const char** res_host) {
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  hipStream_t st = ctx->stream;
  const size_t nb = (size_t)n_bases, tt = (size_t)nt;
  const RGLayout L(nb, fit.sim);
  // b_rg_work: [results | base table 6 nb doubles | sL nb doubles | key nb words | sb nb int32 | error word]
  const size_t w_tab = L.bytes, w_sL = w_tab + nb * 48, w_key = w_sL + nb * 8, w_sb = w_key + nb * 8,
               w_err = up16(w_sb + nb * 4);
  VCP_TRY(vcp_ensure(ctx, ctx->b_rg_work, w_err + 16));
  // b_rg_truth: [sxyz nt*24 | sidx nt*4 | cellof nt*4 | bounds 64 | bounds partials]
  const size_t t_idx = tt * 24, t_cell = t_idx + tt * 4, t_box = up16(t_cell + tt * 4);
  VCP_TRY(vcp_ensure(ctx, ctx->b_rg_truth, t_box + 64 + (size_t)vcp_bounds_parts(nt) * 64));
  char* dw = ctx->b_rg_work.as<char>();
  char* dt = ctx->b_rg_truth.as<char>();
  double* d_tab = reinterpret_cast<double*>(dw + w_tab);
  double* d_sL = reinterpret_cast<double*>(dw + w_sL);
  unsigned long long* d_key = reinterpret_cast<unsigned long long*>(dw + w_key);
  int32_t* d_sb = reinterpret_cast<int32_t*>(dw + w_sb);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(dw + w_err);
  // the pinned stage: [results | Lu nb doubles, then sL in their place | sb nb int32 | error word]
  const size_t s_Lu = L.bytes, s_sb = s_Lu + nb * 8, s_err = up16(s_sb + nb * 4);
  char* stage = static_cast<char*>(vcp_stage(ctx, s_err + 16));
  if (!stage) return vcp_fail(ctx, VCP_ERR_NOMEM, "pinned staging of the per-base results");

  vcp_phase(ctx, fit.sim ? "regs_grid" : "regp_grid");
  VCP_HIP(ctx, hipMemsetAsync(dw, 0, w_err + 16, st));  // results, table, words and the error word
  VCP_LAUNCH(ctx, k_regp_bases, dim3(vcp_blocks(n_bases, RT)), dim3(RT), 0, st, d_src, ns, d_bases, n_bases, d_tab, d_err);
  VCP_HIP(ctx, hipMemcpyAsync(stage + s_Lu, d_tab, nb * 8, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(stage + s_err, d_err, 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  if (*reinterpret_cast<const uint32_t*>(stage + s_err))
    return vcp_fail(ctx, VCP_ERR_INDEX, "a base names a source point outside 0..%lld", (long long)ns - 1);
  // the bases that can make a hypothesis, by length (then by index, so that the order is a fixed one)
  std::vector<double> Lu(nb);
  std::memcpy(Lu.data(), stage + s_Lu, nb * 8);
  std::vector<int32_t> ord;
  for (int32_t b = 0; b < n_bases; b++)
    if (Lu[b] > 0.0 && Lu[b] < INFINITY) ord.push_back(b);
  std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return Lu[x] < Lu[y] || (Lu[x] == Lu[y] && x < y); });
  const int nv = (int)ord.size();
  if (nv > 0) {
    double* h_sL = reinterpret_cast<double*>(stage + s_Lu);
    int32_t* h_sb = reinterpret_cast<int32_t*>(stage + s_sb);
    for (int k = 0; k < nv; k++) {
      h_sL[k] = Lu[ord[k]];
      h_sb[k] = ord[k];
    }
    VCP_HIP(ctx, hipMemcpyAsync(d_sL, h_sL, (size_t)nv * 8, hipMemcpyHostToDevice, st));
    VCP_HIP(ctx, hipMemcpyAsync(d_sb, h_sb, (size_t)nv * 4, hipMemcpyHostToDevice, st));
  }
  RGScan q{};
  q.inlier_dist = inlier_dist;
  {
    bool have = false;
    EpsGrid g{};
    const uint32_t* cellstart = nullptr;
    double* sxyz = reinterpret_cast<double*>(dt);
    VCP_TRY(eg_build_truths<RG_GRID_WG>(
        ctx, d_tgt, (int)nt, inlier_dist,
        TruthGridWork{reinterpret_cast<uint32_t*>(dt + t_cell), sxyz, reinterpret_cast<int32_t*>(dt + t_idx),
                      reinterpret_cast<double*>(dt + t_box), reinterpret_cast<double*>(dt + t_box + 64), &ctx->b_rg_cell},
        &g, &cellstart, &have));
    if (have) {
      q.g = g;
      q.cellstart = cellstart;
      q.sxyz = sxyz;
    }
  }

  vcp_phase(ctx, fit.sim ? "regs_search" : "regp_search");
  int64_t step = 1;
  if (ns > max_landmarks) step = ns / max_landmarks;
  const RGTab tab{d_tab, n_bases};
  unsigned long long* d_nhyp = reinterpret_cast<unsigned long long*>(dw + L.o_nhyp);
  if (nv > 0) {
    const RGSearch a{d_src, step, (int)(ns / step), d_tgt, (int)nt, tab, d_sL, d_sb, nv, fit.len_tol, fit.scale_min,
                     fit.scale_max, mirror ? 2 : 1, q, d_key, d_nhyp};
    if (fit.sim)
      VCP_LAUNCH(ctx, k_regs_search, dim3((unsigned)nt), dim3(RT), 0, st, a);
    else
      VCP_LAUNCH(ctx, k_regp_search, dim3((unsigned)nt), dim3(RT), 0, st, a);
  }

  vcp_phase(ctx, fit.sim ? "regs_final" : "regp_final");
  if (fit.sim)
    VCP_LAUNCH(ctx, k_regs_final, dim3(vcp_blocks(ns, RT), (unsigned)n_bases), dim3(RT), 0, st, d_src, ns, d_tgt, tab, d_key,
               q, reinterpret_cast<double*>(dw + L.o_M), reinterpret_cast<int32_t*>(dw + L.o_score),
               reinterpret_cast<int32_t*>(dw + L.o_pick), reinterpret_cast<uint32_t*>(dw + L.o_inl),
               reinterpret_cast<double*>(dw + L.o_scale));
  else
    VCP_LAUNCH(ctx, k_regp_final, dim3(vcp_blocks(ns, RT), (unsigned)n_bases), dim3(RT), 0, st, d_src, ns, d_tgt, tab, d_key,
               q, reinterpret_cast<double*>(dw + L.o_M), reinterpret_cast<int32_t*>(dw + L.o_score),
               reinterpret_cast<int32_t*>(dw + L.o_pick), reinterpret_cast<uint32_t*>(dw + L.o_inl));
  VCP_HIP(ctx, hipMemcpyAsync(stage, dw, L.bytes, hipMemcpyDeviceToHost, st));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));

  // most inliers, then the higher score, then the lower base; a base without a hypothesis never wins
  const int32_t* sc = reinterpret_cast<const int32_t*>(stage + L.o_score);
  const int32_t* inl = reinterpret_cast<const int32_t*>(stage + L.o_inl);
  int bb = -1;
  for (int b = 0; b < n_bases; b++) {
    if (sc[b] < 0) continue;
    if (bb < 0 || inl[b] > inl[bb] || (inl[b] == inl[bb] && sc[b] > sc[bb])) bb = b;
  }
  if (bb >= 0) {
    std::memcpy(M_best, stage + L.o_M + (size_t)bb * 128, 128);
  } else {
    for (int t = 0; t < 16; t++) M_best[t] = (t % 5 == 0) ? 1.0 : 0.0;
  }
  *best = bb;
  *res_dev = dw;
  *res_host = stage;
  return VCP_OK;
}
}  // namespace

extern "C" {

// Host-side run of the pose arithmetic the kernels execute (same source: rg_base and rg_pose_of are __host__ __device__).
int vcp_selftest_register_pose(const double a[3], const double b[3], const double ti[3], const double tj[3], int f,
                               double Lu_Lv[2], double M[16]) {
  if (!a || !b || !ti || !tj || !Lu_Lv || !M) return VCP_ERR_ARG;
  double r[6];
  rg_base(a, b, r);
  const double vx = tj[0] - ti[0], vy = tj[1] - ti[1];
  Lu_Lv[0] = r[0];
  Lu_Lv[1] = sqrt(vx * vx + vy * vy);
  return rg_pose_of(r, f != 0, ti, tj, M) ? 1 : 0;
}

int vcp_selftest_register_sim_pose(const double a[3], const double b[3], const double ti[3], const double tj[3], int f,
                                   double Lu_Lv_k[3], double M[16]) {
  if (!a || !b || !ti || !tj || !Lu_Lv_k || !M) return VCP_ERR_ARG;
  double r[6], Ms[16], k;
  rg_base(a, b, r);
  const double vx = tj[0] - ti[0], vy = tj[1] - ti[1];
  const bool ok = rg_sim_pose_of(r, f != 0, ti, tj, Ms, &k);
  Lu_Lv_k[0] = r[0];
  Lu_Lv_k[1] = sqrt(vx * vx + vy * vy);
  Lu_Lv_k[2] = k;
  if (ok) std::memcpy(M, Ms, sizeof(Ms));
  return ok ? 1 : 0;
}

}  // extern "C"

namespace {
// The two entry points on device pointers (d_scale: vcp_register_sim_dev only).
int rg_call_dev(vcp_ctx* ctx, const double* d_source, int64_t ns, const double* d_target, int64_t nt, const int32_t* d_bases,
                int32_t n_bases, const RGFit& fit, int mirror, int max_landmarks, double inlier_dist, double M_best[16],
                int32_t* best, double* d_M_all, int32_t* d_score, int32_t* d_inliers, int32_t* d_pick, int64_t* d_n_hyp,
                double* d_scale) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(rg_check(ctx, d_source, ns, d_target, nt, d_bases, n_bases, fit, max_landmarks, inlier_dist, M_best, best));
  const char *rd = nullptr, *rh = nullptr;
  double Mb[16];
  int32_t bb = -1;
  VCP_TRY(rg_run(ctx, d_source, ns, d_target, nt, d_bases, n_bases, fit, mirror, max_landmarks, inlier_dist, Mb, &bb, &rd,
                 &rh));
  const size_t nb = (size_t)n_bases;
  const RGLayout L(nb, fit.sim);
  hipStream_t st = ctx->stream;
  if (d_M_all) VCP_HIP(ctx, hipMemcpyAsync(d_M_all, rd + L.o_M, nb * 128, hipMemcpyDeviceToDevice, st));
  if (d_score) VCP_HIP(ctx, hipMemcpyAsync(d_score, rd + L.o_score, nb * 4, hipMemcpyDeviceToDevice, st));
  if (d_inliers) VCP_HIP(ctx, hipMemcpyAsync(d_inliers, rd + L.o_inl, nb * 4, hipMemcpyDeviceToDevice, st));
  if (d_pick) VCP_HIP(ctx, hipMemcpyAsync(d_pick, rd + L.o_pick, nb * 12, hipMemcpyDeviceToDevice, st));
  if (d_n_hyp) VCP_HIP(ctx, hipMemcpyAsync(d_n_hyp, rd + L.o_nhyp, nb * 8, hipMemcpyDeviceToDevice, st));
  if (fit.sim && d_scale) VCP_HIP(ctx, hipMemcpyAsync(d_scale, rd + L.o_scale, nb * 8, hipMemcpyDeviceToDevice, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  std::memcpy(M_best, Mb, sizeof(Mb));
  *best = bb;
  return VCP_OK;
}

// The two entry points on host pointers (scale: vcp_register_sim only).
int rg_call(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, const int32_t* bases,
            int32_t n_bases, const RGFit& fit, int mirror, int max_landmarks, double inlier_dist, double M_best[16],
            int32_t* best, double* M_all, int32_t* score, int32_t* inliers, int32_t* pick, int64_t* n_hyp, double* scale) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(rg_check(ctx, source, ns, target, nt, bases, n_bases, fit, max_landmarks, inlier_dist, M_best, best));
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // [source ns*24 | target nt*24 | bases n_bases*8]
  const size_t nb = (size_t)n_bases, i_t = (size_t)ns * 24, i_b = i_t + (size_t)nt * 24;
  VCP_TRY(vcp_ensure(ctx, ctx->b_rg_in, i_b + nb * 8));
  char* din = ctx->b_rg_in.as<char>();
  VCP_HIP(ctx, hipMemcpyAsync(din, source, (size_t)ns * 24, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemcpyAsync(din + i_t, target, (size_t)nt * 24, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemcpyAsync(din + i_b, bases, nb * 8, hipMemcpyHostToDevice, st));
  const char *rd = nullptr, *rh = nullptr;
  double Mb[16];
  int32_t bb = -1;
  VCP_TRY(rg_run(ctx, reinterpret_cast<const double*>(din), ns, reinterpret_cast<const double*>(din + i_t), nt,
                 reinterpret_cast<const int32_t*>(din + i_b), n_bases, fit, mirror, max_landmarks, inlier_dist, Mb, &bb, &rd,
                 &rh));
  const RGLayout L(nb, fit.sim);
  if (M_all) std::memcpy(M_all, rh + L.o_M, nb * 128);
  if (score) std::memcpy(score, rh + L.o_score, nb * 4);
  if (inliers) std::memcpy(inliers, rh + L.o_inl, nb * 4);
  if (pick) std::memcpy(pick, rh + L.o_pick, nb * 12);
  if (n_hyp) std::memcpy(n_hyp, rh + L.o_nhyp, nb * 8);
  if (fit.sim && scale) std::memcpy(scale, rh + L.o_scale, nb * 8);
  std::memcpy(M_best, Mb, sizeof(Mb));
  *best = bb;
  return VCP_OK;
}
}  // namespace

extern "C" {

int vcp_register_pairs_dev(vcp_ctx* ctx, const double* d_source, int64_t ns, const double* d_target, int64_t nt,
                           const int32_t* d_bases, int32_t n_bases, double len_tol, int mirror, int max_landmarks,
                           double inlier_dist, double M_best[16], int32_t* best, double* d_M_all, int32_t* d_score,
                           int32_t* d_inliers, int32_t* d_pick, int64_t* d_n_hyp) {
  return rg_call_dev(ctx, d_source, ns, d_target, nt, d_bases, n_bases, RGFit{false, len_tol, 0.0, 0.0}, mirror,
                     max_landmarks, inlier_dist, M_best, best, d_M_all, d_score, d_inliers, d_pick, d_n_hyp, nullptr);
}

int vcp_register_pairs(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                       const int32_t* bases, int32_t n_bases, double len_tol, int mirror, int max_landmarks,
                       double inlier_dist, double M_best[16], int32_t* best, double* M_all, int32_t* score,
                       int32_t* inliers, int32_t* pick, int64_t* n_hyp) {
  return rg_call(ctx, source, ns, target, nt, bases, n_bases, RGFit{false, len_tol, 0.0, 0.0}, mirror, max_landmarks,
                 inlier_dist, M_best, best, M_all, score, inliers, pick, n_hyp, nullptr);
}

int vcp_register_sim_dev(vcp_ctx* ctx, const double* d_source, int64_t ns, const double* d_target, int64_t nt,
                         const int32_t* d_bases, int32_t n_bases, double scale_min, double scale_max, int mirror,
                         int max_landmarks, double inlier_dist, double M_best[16], int32_t* best, double* d_M_all,
                         int32_t* d_score, int32_t* d_inliers, int32_t* d_pick, int64_t* d_n_hyp, double* d_scale) {
  return rg_call_dev(ctx, d_source, ns, d_target, nt, d_bases, n_bases, RGFit{true, 0.0, scale_min, scale_max}, mirror,
                     max_landmarks, inlier_dist, M_best, best, d_M_all, d_score, d_inliers, d_pick, d_n_hyp, d_scale);
}

int vcp_register_sim(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                     const int32_t* bases, int32_t n_bases, double scale_min, double scale_max, int mirror,
                     int max_landmarks, double inlier_dist, double M_best[16], int32_t* best, double* M_all, int32_t* score,
                     int32_t* inliers, int32_t* pick, int64_t* n_hyp, double* scale) {
  return rg_call(ctx, source, ns, target, nt, bases, n_bases, RGFit{true, 0.0, scale_min, scale_max}, mirror, max_landmarks,
                 inlier_dist, M_best, best, M_all, score, inliers, pick, n_hyp, scale);
}

}  // extern "C"
