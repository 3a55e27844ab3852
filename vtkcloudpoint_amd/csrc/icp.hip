// icp.hip -- ICP.go_hell_ICP on MI355X (gfx950).
//
// Per round two launches, no host round trip:
//   k_icp_pass  one fused pass over the data (BaseClass/ICP.cs:195-219 TransPoint, :224-250 FindClosestPointSet,
//               :255-273 means, :38-52 sum p y^T, :126-133 SSE): every thread transforms its points with the
//               current R,T (read from the device-resident state), finds the nearest model point and keeps 16
//               binary64 partial sums; wave shuffle -> workgroup -> one partial row per workgroup.
//   k_icp_step  fixed-order reduction of the partial rows (bitwise reproducible, no float atomics), then ONE
//               thread solves Horn's closed form (the INTENDED arithmetic of :53-124), applies
//               the stop rule (:149,:180) and composes R <- R1 R, T <- R1 T + T1 (:149-177) in the state.
// The host enqueues rounds in batches of 8 and reads the 424-byte state back once per batch; kernels of rounds
// after the stop see state.done and return at once.
// Multi-start (vcp_icp_multistart): H independent states run side by side -- blockIdx.y of the pass selects the state
// and its slice of partial rows, k_icp_step runs one workgroup per state, and each state's partition into workgroups and
// reduction order are those of a single run, so every pose's bits are independent of the batch.  k_icpms_score then
// counts, per pose, the source points vcp_match would call matched.
//
// Nearest neighbour: the model index is wave-uniform, so model points come through the scalar cache, four per
// trip.  Distances are first screened in binary32 (three FMAs per pair) with a rigorous rounding bound; only model points whose
// binary32 distance is within that bound of the smallest are re-evaluated in binary64, in index order with the
// C#'s strict `<` -- the chosen index is bit-identical to a full binary64 scan.
// Algorithmic bytes: 24 B per data point per round; at 1M x 100 the pass is VALU bound, not HBM bound.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "match.hpp"
#include "nngrid.hpp"
#include "reduce.hpp"
#include "vcp_ctx.hpp"

namespace {

constexpr int ITPB = 256;
constexpr int ICP_MAX_BLOCKS = 1024;  // part of the sums' bits: tests/icp_sums_ref.py restates it (MAX_BLOCKS), change both
constexpr int ICP_BATCH = 8;  // rounds enqueued per host synchronisation
constexpr int ICPMS_MAX_POSES = 4096;

enum { MODE_REFERENCE = 0, MODE_VTK = 1, MODE_SUMS_ONLY = 2 };

struct IcpState {
  double R[9], T[3];
  double d, pre_d;
  double sums[16];
  double cen[3], mmax;  // centre of the model's bounding box and its half extent: frame and scale of the screening
  double V[16];         // eigenvector basis of the last Horn solve (all zero = none yet)
  int round, done, failed;
  int starved;     // gated runs: rounds that kept fewer than min_pairs pairs (R, T, V untouched by them)
  long long kept;  // gated runs: pairs the last pass kept
};

// What a gated pass reads beside the state (vcp.h, vcp_icp_gated): the schedule on the device (round r, 1-based, uses
// gates[min(r, n_gates) - 1]; the state's round counter says which), one kept count per workgroup next to its partial
// row, and optionally the per-point verdict.
struct GateArgs {
  const double* gates;
  int n_gates;
  uint32_t* pkept;  // [poses][workgroups]
  uint8_t* keep;    // [nd] or NULL
};
struct NoGate {};
// Similarity ICP (vcp.h, "similarity ICP"): the gated pass with two more columns, sum |p|^2 at 16 and sum |y|^2 at 17,
// through the same tree.  A type of its own: the kernels of GateArgs stay the 16-wide ones they were.
struct SimGate {
  GateArgs g;
};
// columns of a pass's rows
template <class G>
constexpr int icp_ncol = std::is_same<G, SimGate>::value ? 18 : 16;

// Trimmed ICP (vcp.h, "trimmed ICP"): a round keeps the m landmarks with the smallest 96-bit keys [K(dd) | index].
// Three steps per round and pose: a pass that runs the NN search and stores K(dd) and the index found (G = TrimDist),
// a radix select of the rank-m key (k_icpt_select_wg, or k_icpt_hist x 12 + k_icpt_select_fin), and the sums pass
// (G = TrimSum), which reads both back and keeps "key <= the selected one" where the gated pass tests the distance.
struct TrimSel {
  unsigned long long key;  // K(dd) of the kept pair with the largest key: thr's bit pattern (all ones: NaN)
  uint32_t idx, pad;       // and its landmark
};
struct TrimArgs {
  const double* share;  // the keep schedule on the device: round r (1-based) uses share[min(r, n_share) - 1]
  int n_share;
  long long m_fixed;  // > 0: the keep count itself (vcp_icp_sums_trimmed)
  unsigned long long* key;  // [poses][L]
  int32_t* nn;              // [poses][L]
  TrimSel* sel;             // [poses]
  uint32_t* pkept;          // [poses][workgroups]
  uint8_t* keep;            // [L] or NULL
};
struct TrimDist {
  TrimArgs a;
};
struct TrimSum {
  TrimArgs a;
};
// Unique-correspondence ICP (vcp.h, "unique-correspondence ICP"): of the landmarks that share a nearest target, only the
// one with the smallest 96-bit key [K(dd) | index] -- the target's WINNER -- may enter the sums; the gate then decides
// on the winner as it does in the gated pass.  Three steps per round and pose: a pass that runs the NN search, stores
// K(dd) and the index found and takes the 64-bit minimum of K(dd) in the slot of (pose, target) (G = UniqDist); the tie
// pass k_icpu_tie, the 32-bit minimum of the landmark among those whose K equals the slot's; and the sums pass
// (G = UniqSum), which keeps "my key and my index are the slot's, and the gate keeps me".  A slot is 12 bytes, two
// arrays: skey [poses][nt] and sidx [poses][nt], all ones between rounds.
struct UniqArgs {
  const double* gates;  // the schedule on the device, as GateArgs'
  int n_gates;
  int nt;                    // targets: slots per pose
  unsigned long long* key;   // [poses][L]
  int32_t* nn;               // [poses][L]
  unsigned long long* skey;  // [poses][nt]
  uint32_t* sidx;            // [poses][nt]
  uint32_t* pkept;           // [poses][workgroups]
  uint32_t* plost;           // [poses][workgroups]: pairs that are not their target's winner
  uint8_t* keep;             // [L] or NULL: 1 kept, 0 winner dropped by the gate, 2 not the winner
};
struct UniqDist {
  UniqArgs a;
};
struct UniqSum {
  UniqArgs a;
};
__device__ __forceinline__ uint8_t* keep_of(const GateArgs& g) { return g.keep; }
__device__ __forceinline__ uint8_t* keep_of(const TrimSum& t) { return t.a.keep; }
__device__ __forceinline__ uint8_t* keep_of(const SimGate& s) { return s.g.keep; }
__device__ __forceinline__ uint8_t* keep_of(const UniqSum& u) { return u.a.keep; }
__device__ __forceinline__ uint32_t* pkept_of(const GateArgs& g) { return g.pkept; }
__device__ __forceinline__ uint32_t* pkept_of(const TrimSum& t) { return t.a.pkept; }
__device__ __forceinline__ uint32_t* pkept_of(const SimGate& s) { return s.g.pkept; }
__device__ __forceinline__ uint32_t* pkept_of(const UniqSum& u) { return u.a.pkept; }
// K(dd): dd's bit pattern (dd >= +0, so the unsigned order is the numeric one, +inf last of the numbers), NaN above all
__device__ __forceinline__ unsigned long long trim_key(double dd) {
  return dd != dd ? ~0ull : (unsigned long long)__double_as_longlong(dd);
}

// bounding box of the model -> centre and half extent in the nst states (single workgroup: models are small).  A model
// with non-finite coordinates gets an infinite scale: every data point is then resolved in binary64.
__global__ __launch_bounds__(ITPB) void k_model_frame(const double* __restrict__ m, int64_t nm, IcpState* __restrict__ st,
                                                     int nst) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (int64_t j = threadIdx.x; j < nm; j += ITPB) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double v = m[3 * j + a];
      if (!(fabs(v) <= 1.7976931348623157e308)) bad = true;
      lo[a] = fmin(lo[a], v);
      hi[a] = fmax(hi[a], v);
    }
  }
  __shared__ double sl[ITPB / 64][3], sh[ITPB / 64][3];
  __shared__ int sbad;
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  if (bad) sbad = 1;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double l = wave_min(lo[a]), h = wave_max(hi[a]);
    if (lane == 0) {
      sl[w][a] = l;
      sh[w][a] = h;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double mm = 0.0, cen[3];
    for (int a = 0; a < 3; a++) {
      double l = sl[0][a], h = sh[0][a];
      for (int k = 1; k < ITPB / 64; k++) {
        l = fmin(l, sl[k][a]);
        h = fmax(h, sh[k][a]);
      }
      const double c = 0.5 * l + 0.5 * h;
      cen[a] = sbad ? 0.0 : c;
      mm = fmax(mm, fmax(h - c, c - l));
    }
    for (int k = 0; k < nst; k++) {
      for (int a = 0; a < 3; a++) st[k].cen[a] = cen[a];
      st[k].mmax = sbad ? INFINITY : mm;
    }
  }
}

// screening copy of the model in the centred frame: (m - c, |m - c|^2 / 2) in binary32, one 16-byte load per point
__global__ __launch_bounds__(ITPB) void k_model32(const double* __restrict__ m, int64_t nm, const IcpState* __restrict__ st,
                                                 float4* __restrict__ o) {
  int64_t j = (int64_t)blockIdx.x * ITPB + threadIdx.x;
  if (j >= nm) return;
  const double a = m[3 * j] - st->cen[0], b = m[3 * j + 1] - st->cen[1], c = m[3 * j + 2] - st->cen[2];
  o[j] = make_float4((float)a, (float)b, (float)c, (float)(0.5 * (a * a + b * b + c * c)));
}

// TB = threads per workgroup (64 for small data sets, so that they spread over more CUs).  TILED: the screening
// copy of the model is staged through LDS in tiles of MTILE points (every lane reads the same address: an LDS
// broadcast).  The scalar-cache path is the faster one while the model fits that cache (C3: 100 points); a model
// of thousands of points (ICP of cluster centroids against the truth list, MainForm.ICP's real use) makes every
// scalar load an L2 round trip, 30x slower than the tiled form.
// NNMODE 2: the model has been binned (nngrid.hpp): every lane searches the cells round its own transformed point --
// O(1) candidates per data point instead of the whole model, same exact binary64 decision and tie rule.
struct StepArgs {
  long long nd;
  double tol;
  int stop_rule, max_iter, mode;
};

constexpr int MTILE = 1024;
// The gate of the pass a gated kernel runs now, and a workgroup's kept count written next to its partial row (wave
// shuffle, then the waves in order: integers, exact in any order).
__device__ __forceinline__ double gate_now(const GateArgs& ga, const IcpState* st) {
  return ga.gates[min(st->round + 1, ga.n_gates) - 1];
}
__device__ __forceinline__ double gate_now(const SimGate& sg, const IcpState* st) { return gate_now(sg.g, st); }
__device__ __forceinline__ double gate_now(const UniqSum& us, const IcpState* st) {
  return us.a.gates[min(st->round + 1, us.a.n_gates) - 1];
}
// The keep count of the round a trimmed kernel runs now: min(L, ceil(f * L)), one multiplication; f in (0, 1] (checked
// on the host), so the count lies in [1, L].
__device__ __forceinline__ long long trim_m(const TrimArgs& a, const IcpState* st, long long L) {
  if (a.m_fixed > 0) return a.m_fixed;
  const double f = a.share[min(st->round + 1, a.n_share) - 1];
  const long long m = (long long)ceil(f * (double)L);
  return m < L ? m : L;
}
template <int TB>
__device__ __forceinline__ void block_count(uint32_t c, uint32_t* __restrict__ out) {
  __shared__ uint32_t sk[TB / 64];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < TB / 64; w++) t += sk[w];
    *out = t;
  }
}

// GATED (G = GateArgs): a pair whose distance sqrt(dd) is >= the round's gate adds +0.0 to each of the 16 rows at its
// own place in the tree, which therefore stays the ungated one; dd is the SSE term.  A NaN dd compares false: kept.
template <int TB, int NNMODE, class G>
__device__ __forceinline__ void icp_pass_body(const double* __restrict__ model, const float4* __restrict__ model32,
                                              int nm, const double* __restrict__ data, int64_t nd,
                                              const IcpState* __restrict__ st, double* __restrict__ partial,
                                              int32_t* __restrict__ nn, const NNGrid& ng, const G& ga) {
  constexpr bool SIM = std::is_same<G, SimGate>::value;  // GATED with the two columns of the scale
  constexpr bool GATED = std::is_same<G, GateArgs>::value || SIM;
  constexpr int NS = icp_ncol<G>;
  // TDIST: the search alone, K(dd) and the index stored per landmark; TSUM: no search, the stored index, and the sums
  // of the landmarks whose key is <= the selected one
  constexpr bool TDIST = std::is_same<G, TrimDist>::value, TSUM = std::is_same<G, TrimSum>::value;
  // UDIST / USUM: the two passes of a unique-correspondence round; DIST / RSUM: what they share with the trimmed ones
  // (DIST: the search alone, key and index stored; RSUM: no search, the stored index)
  constexpr bool UDIST = std::is_same<G, UniqDist>::value, USUM = std::is_same<G, UniqSum>::value;
  constexpr bool DIST = TDIST || UDIST, RSUM = TSUM || USUM;
  st += blockIdx.y;  // the pose's state and partial rows (gridDim.y = 1 outside vcp_icp_multistart)
  partial += (size_t)blockIdx.y * gridDim.x * NS;
  if (st->done) return;
  double gate = 0.0;
  uint32_t nkept = 0, nlost = 0;
  if constexpr (GATED || USUM) gate = gate_now(ga, st);
  unsigned long long* tkey = nullptr;
  int32_t* tnn = nullptr;
  unsigned long long thrk = 0;
  uint32_t thri = 0;
  if constexpr (DIST || RSUM) {
    tkey = ga.a.key + (size_t)blockIdx.y * (size_t)nd;
    tnn = ga.a.nn + (size_t)blockIdx.y * (size_t)nd;
  }
  if constexpr (TSUM) {
    thrk = ga.a.sel[blockIdx.y].key;
    thri = ga.a.sel[blockIdx.y].idx;
  }
  constexpr bool TILED = NNMODE == 1, GRID = NNMODE == 2;
  __shared__ float4 tile[TILED && !RSUM ? MTILE : 1];
  double R[9], T[3];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = st->R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) T[k] = st->T[k];
  // binary32 screening on the score h_j - q.m_j (= (|q - m_j|^2 - |q|^2) / 2, h_j = |m_j|^2 / 2), q and m taken
  // relative to the centre of the model's bounding box (the score differences are translation invariant): three
  // FMAs per model point.  With S = a bound on every |coordinate| involved (this lane's |q - c| and the model's half
  // extent) and u = 2^-24 the computed score is within 27 u S^2 of the exact one (input conversions 9 u S^2, h_j
  // 4.5 u S^2, three fused roundings 13.5 u S^2), so a model point can be the binary64 winner only if
  // score <= best score + 54 u S^2; 2^-17 S^2 = 128 u S^2 is used.  The bound is per data point.
  const double cen0 = st->cen[0], cen1 = st->cen[1], cen2 = st->cen[2], mmax = st->mmax;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) s[k] = 0.0;
  // GRID: nng::NNG consecutive lanes work one data point (they split the rows of its search block)
  constexpr int LPQ = GRID ? nng::NNG : 1;
  const int sub = GRID ? (int)(threadIdx.x & (LPQ - 1)) : 0;
  for (int64_t base = (int64_t)blockIdx.x * TB; base < nd * LPQ; base += (int64_t)gridDim.x * TB) {  // uniform trip count
    const int64_t i = (base + threadIdx.x) / LPQ;
    const bool live = i < nd;
    const int64_t il = live ? i : nd - 1;  // idle lanes of the last workgroup recompute the last point, unused
    const double d0 = data[3 * il], d1 = data[3 * il + 1], d2 = data[3 * il + 2];
    // TransPoint: r = R*p accumulated k ascending from 0 (Matrix.StupidMultiply), then + T
    double p[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      double acc = 0.0;
      acc += R[3 * r] * d0;
      acc += R[3 * r + 1] * d1;
      acc += R[3 * r + 2] * d2;
      p[r] = acc + T[r];
    }
    int order = 0;
    if constexpr (RSUM) {
      order = tnn[il];
    } else if (GRID) {
      double bestv;
      nng::query<false>(ng, p, sub, order, bestv);
    } else {
    const double pc0 = p[0] - cen0, pc1 = p[1] - cen1, pc2 = p[2] - cen2;
    const float q0 = (float)pc0, q1 = (float)pc1, q2 = (float)pc2;
    const double S = fmax(mmax, fmax(fabs(pc0), fmax(fabs(pc1), fabs(pc2))));
    // 2^-17 S^2, rounded up (NaN -> all candidates; also outside binary32's normal range, where the relative rounding
    // model behind the bound does not hold)
    const float tol2r = (float)(S * S * 7.62939453125e-06) * 1.0001f;
    const float tol2 = ((float)(S * S) < 1.0e37f && tol2r >= 1.0e-30f) ? tol2r : NAN;
    // pass 1 (binary32): smallest and second smallest screened score, four model points per trip
    float b1 = INFINITY, b2 = INFINITY;
    int j1 = 0;
    int j = 0;
    if (TILED) {
      for (int t0 = 0; t0 < nm; t0 += MTILE) {
        const int cnt = min(MTILE, nm - t0);
        __syncthreads();  // the previous tile has been consumed
        for (int k = threadIdx.x; k < cnt; k += TB) tile[k] = model32[t0 + k];
        __syncthreads();
        int u = 0;
        for (; u + 3 < cnt; u += 4) {
          float4 mm[4];
#pragma unroll
          for (int v = 0; v < 4; v++) mm[v] = tile[u + v];
#pragma unroll
          for (int v = 0; v < 4; v++) {
            const float sc = __builtin_fmaf(-q0, mm[v].x, __builtin_fmaf(-q1, mm[v].y, __builtin_fmaf(-q2, mm[v].z, mm[v].w)));
            const bool lt = sc < b1;
            b2 = lt ? b1 : fminf(b2, sc);
            j1 = lt ? t0 + u + v : j1;
            b1 = lt ? sc : b1;
          }
        }
        for (; u < cnt; u++) {
          const float4 m4 = tile[u];
          const float sc = __builtin_fmaf(-q0, m4.x, __builtin_fmaf(-q1, m4.y, __builtin_fmaf(-q2, m4.z, m4.w)));
          const bool lt = sc < b1;
          b2 = lt ? b1 : fminf(b2, sc);
          j1 = lt ? t0 + u : j1;
          b1 = lt ? sc : b1;
        }
      }
      j = nm;
    }
    for (; j + 3 < nm; j += 4) {
      float4 mm[4];
#pragma unroll
      for (int u = 0; u < 4; u++) mm[u] = model32[j + u];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const float sc = __builtin_fmaf(-q0, mm[u].x, __builtin_fmaf(-q1, mm[u].y, __builtin_fmaf(-q2, mm[u].z, mm[u].w)));
        const bool lt = sc < b1;
        b2 = lt ? b1 : fminf(b2, sc);
        j1 = lt ? j + u : j1;
        b1 = lt ? sc : b1;
      }
    }
    for (; j < nm; j++) {
      const float4 m4 = model32[j];
      const float sc = __builtin_fmaf(-q0, m4.x, __builtin_fmaf(-q1, m4.y, __builtin_fmaf(-q2, m4.z, m4.w)));
      const bool lt = sc < b1;
      b2 = lt ? b1 : fminf(b2, sc);
      j1 = lt ? j : j1;
      b1 = lt ? sc : b1;
    }
    order = j1;
    const bool amb = !(b2 > b1 + tol2);
    if (TILED) {
      // second sweep over the tiles for the lanes whose screening left more than one candidate; the whole
      // workgroup walks the tiles (uniform barriers), only ambiguous lanes look at them
      if (__syncthreads_or(amb ? 1 : 0)) {
        const float lim = b1 + tol2;
        const bool all = !(lim == lim);  // non-finite bound: every model point is a candidate
        double best = INFINITY;
        bool have = false;
        if (amb) order = 0;
        for (int t0 = 0; t0 < nm; t0 += MTILE) {
          const int cnt = min(MTILE, nm - t0);
          __syncthreads();
          for (int k = threadIdx.x; k < cnt; k += TB) tile[k] = model32[t0 + k];
          __syncthreads();
          if (!amb) continue;
          for (int u = 0; u < cnt; u += 4) {
            float sc[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
              const float4 m4 = tile[min(u + v, cnt - 1)];
              sc[v] = __builtin_fmaf(-q0, m4.x, __builtin_fmaf(-q1, m4.y, __builtin_fmaf(-q2, m4.z, m4.w)));
            }
#pragma unroll
            for (int v = 0; v < 4; v++) {
              if (u + v >= cnt || !(sc[v] <= lim || !(sc[v] == sc[v]) || all)) continue;
              const int jj = t0 + u + v;
              const double e0 = p[0] - model[3 * jj], e1 = p[1] - model[3 * jj + 1], e2 = p[2] - model[3 * jj + 2];
              const double dd = e0 * e0 + e1 * e1 + e2 * e2;
              if (!have || dd < best) {
                best = dd;
                order = jj;
                have = true;
              }
            }
          }
        }
      }
    } else if (amb) {
      // more than one candidate within the bound (or non-finite values): exact binary64 among the candidates, in
      // index order, strict `<` -- FindClosestPointSet's rule (the C# seeds with model[0] and replaces on `<`, so
      // the lowest index among the exact minima wins; every exact minimum is a candidate by the bound)
      const float lim = b1 + tol2;
      double best = INFINITY;
      bool have = false;
      order = 0;
      for (int jj = 0; jj < nm; jj++) {
        const float4 m4 = model32[jj];
        const float sc = __builtin_fmaf(-q0, m4.x, __builtin_fmaf(-q1, m4.y, __builtin_fmaf(-q2, m4.z, m4.w)));
        if (sc <= lim || !(sc == sc) || !(lim == lim)) {
          const double e0 = p[0] - model[3 * jj], e1 = p[1] - model[3 * jj + 1], e2 = p[2] - model[3 * jj + 2];
          const double dd = e0 * e0 + e1 * e1 + e2 * e2;
          if (!have || dd < best) {
            best = dd;
            order = jj;
            have = true;
          }
        }
      }
    }
    }  // !GRID
    if (!live || sub != 0) continue;  // one lane of the group carries the point into the sums
    if (nn) nn[i] = order;
    const double y0 = model[3 * order], y1 = model[3 * order + 1], y2 = model[3 * order + 2];
    const double y[3] = {y0, y1, y2};
    if constexpr (DIST) {
      const double e0 = p[0] - y0, e1 = p[1] - y1, e2 = p[2] - y2;
      const unsigned long long k = trim_key(e0 * e0 + e1 * e1 + e2 * e2);
      tkey[i] = k;
      tnn[i] = order;
      if constexpr (UDIST) atomicMin(ga.a.skey + (size_t)blockIdx.y * (size_t)ga.a.nt + (size_t)order, k);
    } else if constexpr (GATED || RSUM) {
      const double e0 = p[0] - y0, e1 = p[1] - y1, e2 = p[2] - y2;
      const double dd = e0 * e0 + e1 * e1 + e2 * e2;
      bool kp;
      uint8_t code;  // what keep[] receives
      if constexpr (GATED) {
        kp = !(sqrt(dd) >= gate);
        code = kp ? 1 : 0;
      } else if constexpr (USUM) {
        const size_t sl = (size_t)blockIdx.y * (size_t)ga.a.nt + (size_t)order;
        const bool win = tkey[i] == ga.a.skey[sl] && (uint32_t)i == ga.a.sidx[sl];
        kp = win && !(sqrt(dd) >= gate);
        nlost += win ? 0u : 1u;
        code = win ? (kp ? 1 : 0) : 2;
      } else {
        const unsigned long long k = tkey[i];
        kp = k < thrk || (k == thrk && (uint32_t)i <= thri);
        code = kp ? 1 : 0;
      }
      if (keep_of(ga)) keep_of(ga)[i] = code;
      nkept += kp ? 1u : 0u;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        s[r] += kp ? p[r] : 0.0;
        s[3 + r] += kp ? y[r] : 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) s[6 + 3 * r + c] += kp ? p[r] * y[c] : 0.0;
      }
      s[15] += kp ? dd : 0.0;
      if constexpr (SIM) {
        s[16] += kp ? (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2] : 0.0;
        s[17] += kp ? (y0 * y0 + y1 * y1) + y2 * y2 : 0.0;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        s[r] += p[r];
        s[3 + r] += y[r];
#pragma unroll
        for (int c = 0; c < 3; c++) s[6 + 3 * r + c] += p[r] * y[c];
      }
      const double e0 = p[0] - y0, e1 = p[1] - y1, e2 = p[2] - y2;
      s[15] += e0 * e0 + e1 * e1 + e2 * e2;
    }
  }
  if constexpr (!DIST) block_fold<TB>(s, FoldSum(), partial + (size_t)blockIdx.x * NS);
  if constexpr (GATED || RSUM) block_count<TB>(nkept, pkept_of(ga) + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
  if constexpr (USUM) {
    __syncthreads();  // block_count's LDS words are free again
    block_count<TB>(nlost, ga.a.plost + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
  }
}

template <int TB, int NNMODE>
__global__ __launch_bounds__(TB) void k_icp_pass(const double* __restrict__ model, const float4* __restrict__ model32,
                                                int nm, const double* __restrict__ data, int64_t nd,
                                                const IcpState* __restrict__ st, double* __restrict__ partial,
                                                int32_t* __restrict__ nn, NNGrid ng) {
  icp_pass_body<TB, NNMODE>(model, model32, nm, data, nd, st, partial, nn, ng, NoGate());
}
template <int TB, int NNMODE>
__global__ __launch_bounds__(TB) void k_icp_pass_gated(const double* __restrict__ model,
                                                      const float4* __restrict__ model32, int nm,
                                                      const double* __restrict__ data, int64_t nd,
                                                      const IcpState* __restrict__ st, double* __restrict__ partial,
                                                      int32_t* __restrict__ nn, NNGrid ng, GateArgs ga) {
  icp_pass_body<TB, NNMODE>(model, model32, nm, data, nd, st, partial, nn, ng, ga);
}

template <int TB, int NNMODE>
__global__ __launch_bounds__(TB) void k_icp_pass_sim(const double* __restrict__ model,
                                                    const float4* __restrict__ model32, int nm,
                                                    const double* __restrict__ data, int64_t nd,
                                                    const IcpState* __restrict__ st, double* __restrict__ partial,
                                                    int32_t* __restrict__ nn, NNGrid ng, SimGate ga) {
  icp_pass_body<TB, NNMODE>(model, model32, nm, data, nd, st, partial, nn, ng, ga);
}

// ---- small models (nm <= 512: MainForm's 100 truths, C3) ---------------------------------------------------
// The same pass with the screening loop reshaped for the VALU, which bounds it at 1 M x 100:
//   * every lane works TWO data points at once, so the three FMAs of a score are packed binary32 operations
//     (v_pk_fma_f32: two points per instruction against the one wave-uniform model point from the scalar cache);
//   * the model index rides in the low `ib` mantissa bits of the score, so "smallest and second smallest score and
//     the index of the smallest" is one v_and_or, one v_med3 and one v_min per pair instead of a compare, a min and
//     three selects.  Replacing the low bits moves a score by at most 2^(ib-24) of its magnitude (<= 4.5 S^2); the
//     ambiguity bound grows by twice that: (54 + 9 * 2^ib) u S^2, rounded up to a power of two on the host (tolk).
//     A point whose two best scores are closer than the bound is decided in binary64 exactly as before.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// min of two scores as ONE instruction: fminf() first quiets both operands (a v_max x, x each) for IEEE signalling-NaN
// semantics, doubling the cost of the hottest statement; NaN scores never reach the result (see tol2 below)
__device__ __forceinline__ float min_raw(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

template <int TB, class G>
__device__ __forceinline__ void icp_pass_small_body(const double* __restrict__ model, const float4* __restrict__ model32,
                                                    int nm, const double* __restrict__ data, int64_t nd,
                                                    const IcpState* __restrict__ st, double* __restrict__ partial,
                                                    int32_t* __restrict__ nn, uint32_t imask, double tolk, const G& ga) {
  constexpr bool SIM = std::is_same<G, SimGate>::value;  // as in icp_pass_body
  constexpr bool GATED = std::is_same<G, GateArgs>::value || SIM;
  constexpr int NS = icp_ncol<G>;
  constexpr bool TDIST = std::is_same<G, TrimDist>::value, TSUM = std::is_same<G, TrimSum>::value;
  // UDIST / USUM: the two passes of a unique-correspondence round; DIST / RSUM: what they share with the trimmed ones
  // (DIST: the search alone, key and index stored; RSUM: no search, the stored index)
  constexpr bool UDIST = std::is_same<G, UniqDist>::value, USUM = std::is_same<G, UniqSum>::value;
  constexpr bool DIST = TDIST || UDIST, RSUM = TSUM || USUM;
  st += blockIdx.y;  // the pose's state and partial rows (gridDim.y = 1 outside vcp_icp_multistart)
  partial += (size_t)blockIdx.y * gridDim.x * NS;
  if (st->done) return;
  double gate = 0.0;
  uint32_t nkept = 0, nlost = 0;
  if constexpr (GATED || USUM) gate = gate_now(ga, st);
  unsigned long long* tkey = nullptr;
  int32_t* tnn = nullptr;
  unsigned long long thrk = 0;
  uint32_t thri = 0;
  if constexpr (DIST || RSUM) {
    tkey = ga.a.key + (size_t)blockIdx.y * (size_t)nd;
    tnn = ga.a.nn + (size_t)blockIdx.y * (size_t)nd;
  }
  if constexpr (TSUM) {
    thrk = ga.a.sel[blockIdx.y].key;
    thri = ga.a.sel[blockIdx.y].idx;
  }
  double R[9], T[3];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = st->R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) T[k] = st->T[k];
  const double cen0 = st->cen[0], cen1 = st->cen[1], cen2 = st->cen[2], mmax = st->mmax;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) s[k] = 0.0;
  const int64_t half = (nd + 1) >> 1;  // lane v works points v and v + half
  for (int64_t base = (int64_t)blockIdx.x * TB; base < half; base += (int64_t)gridDim.x * TB) {  // uniform trip count
    const int64_t v = base + threadIdx.x;
    int64_t idx[2] = {v, v + half};
    bool live[2] = {v < half, v < half && v + half < nd};
    double p[2][3];
    float q[2][3], tol2[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int64_t il = live[h] ? idx[h] : nd - 1;  // idle slots recompute the last point, unused
      const double d0 = data[3 * il], d1 = data[3 * il + 1], d2 = data[3 * il + 2];
      // TransPoint: r = R*p accumulated k ascending from 0 (Matrix.StupidMultiply), then + T
#pragma unroll
      for (int r = 0; r < 3; r++) {
        double acc = 0.0;
        acc += R[3 * r] * d0;
        acc += R[3 * r + 1] * d1;
        acc += R[3 * r + 2] * d2;
        p[h][r] = acc + T[r];
      }
      const double pc0 = p[h][0] - cen0, pc1 = p[h][1] - cen1, pc2 = p[h][2] - cen2;
      q[h][0] = (float)pc0;
      q[h][1] = (float)pc1;
      q[h][2] = (float)pc2;
      const double S = fmax(mmax, fmax(fabs(pc0), fmax(fabs(pc1), fabs(pc2))));
      const float t2 = (float)(S * S * tolk) * 1.0001f;
      // scores are bounded by 4.5 S^2: beyond binary32 range (or NaN) the point goes to the exact scan
      // outside binary32's normal range the rounding model behind tolk does not hold (underflow: absolute errors of
      // 2^-149; overflow: inf scores): NaN = every candidate goes through the binary64 comparison
      tol2[h] = ((float)(S * S) < 1.0e37f && t2 >= 1.0e-30f) ? t2 : NAN;
    }
    float b1[2] = {INFINITY, INFINITY}, b2[2] = {INFINITY, INFINITY};
    if constexpr (!RSUM) {
    const f32x2 nq0 = {-q[0][0], -q[1][0]}, nq1 = {-q[0][1], -q[1][1]}, nq2 = {-q[0][2], -q[1][2]};
    // the mask lives in a VGPR so that (score & keep) | j is ONE v_and_or_b32 (a VOP3 reads one scalar operand: j)
    uint32_t keep;
    asm volatile("v_mov_b32 %0, %1" : "=v"(keep) : "s"(~imask));
    int j = 0;
    for (; j + 1 < nm; j += 2) {
      const float4 ma = model32[j], mb = model32[j + 1];
      const f32x2 sa = __builtin_elementwise_fma(nq0, (f32x2)(ma.x), __builtin_elementwise_fma(nq1, (f32x2)(ma.y),
                       __builtin_elementwise_fma(nq2, (f32x2)(ma.z), (f32x2)(ma.w))));
      const f32x2 sb = __builtin_elementwise_fma(nq0, (f32x2)(mb.x), __builtin_elementwise_fma(nq1, (f32x2)(mb.y),
                       __builtin_elementwise_fma(nq2, (f32x2)(mb.z), (f32x2)(mb.w))));
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float ta = __uint_as_float((__float_as_uint(sa[h]) & keep) | (uint32_t)j);
        const float tb = __uint_as_float((__float_as_uint(sb[h]) & keep) | (uint32_t)(j + 1));
        b2[h] = __builtin_amdgcn_fmed3f(b1[h], b2[h], ta);
        b1[h] = min_raw(b1[h], ta);
        b2[h] = __builtin_amdgcn_fmed3f(b1[h], b2[h], tb);
        b1[h] = min_raw(b1[h], tb);
      }
    }
    if (j < nm) {
      const float4 ma = model32[j];
      const f32x2 sa = __builtin_elementwise_fma(nq0, (f32x2)(ma.x), __builtin_elementwise_fma(nq1, (f32x2)(ma.y),
                       __builtin_elementwise_fma(nq2, (f32x2)(ma.z), (f32x2)(ma.w))));
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float ta = __uint_as_float((__float_as_uint(sa[h]) & keep) | (uint32_t)j);
        b2[h] = __builtin_amdgcn_fmed3f(b1[h], b2[h], ta);
        b1[h] = min_raw(b1[h], ta);
      }
    }
    }  // !RSUM
#pragma unroll
    for (int h = 0; h < 2; h++) {
      int order = (int)(__float_as_uint(b1[h]) & imask);
      const bool amb = !RSUM && !(b2[h] > b1[h] + tol2[h]);
      if constexpr (RSUM) order = tnn[live[h] ? idx[h] : nd - 1];
      if (amb) {
        // more than one candidate within the bound (or non-finite values): exact binary64 among the candidates, in
        // index order, strict `<` -- FindClosestPointSet's rule (lowest index among the exact minima)
        const float lim = b1[h] + tol2[h];
        double best = INFINITY;
        bool have = false;
        order = 0;
        for (int jj = 0; jj < nm; jj++) {
          const float4 m4 = model32[jj];
          const float sc = __builtin_fmaf(-q[h][0], m4.x, __builtin_fmaf(-q[h][1], m4.y, __builtin_fmaf(-q[h][2], m4.z, m4.w)));
          if (sc <= lim || !(sc == sc) || !(lim == lim)) {
            const double e0 = p[h][0] - model[3 * jj], e1 = p[h][1] - model[3 * jj + 1], e2 = p[h][2] - model[3 * jj + 2];
            const double dd = e0 * e0 + e1 * e1 + e2 * e2;
            if (!have || dd < best) {
              best = dd;
              order = jj;
              have = true;
            }
          }
        }
      }
      if (!live[h]) continue;
      if (nn) nn[idx[h]] = order;
      const double y0 = model[3 * order], y1 = model[3 * order + 1], y2 = model[3 * order + 2];
      const double y[3] = {y0, y1, y2};
      if constexpr (DIST) {
        const double e0 = p[h][0] - y0, e1 = p[h][1] - y1, e2 = p[h][2] - y2;
        const unsigned long long k = trim_key(e0 * e0 + e1 * e1 + e2 * e2);
        tkey[idx[h]] = k;
        tnn[idx[h]] = order;
        if constexpr (UDIST) atomicMin(ga.a.skey + (size_t)blockIdx.y * (size_t)ga.a.nt + (size_t)order, k);
      } else if constexpr (GATED || RSUM) {
        const double e0 = p[h][0] - y0, e1 = p[h][1] - y1, e2 = p[h][2] - y2;
        const double dd = e0 * e0 + e1 * e1 + e2 * e2;
        bool kp;
        uint8_t code;  // what keep[] receives
        if constexpr (GATED) {
          kp = !(sqrt(dd) >= gate);
          code = kp ? 1 : 0;
        } else if constexpr (USUM) {
          const size_t sl = (size_t)blockIdx.y * (size_t)ga.a.nt + (size_t)order;
          const bool win = tkey[idx[h]] == ga.a.skey[sl] && (uint32_t)idx[h] == ga.a.sidx[sl];
          kp = win && !(sqrt(dd) >= gate);
          nlost += win ? 0u : 1u;
          code = win ? (kp ? 1 : 0) : 2;
        } else {
          const unsigned long long k = tkey[idx[h]];
          kp = k < thrk || (k == thrk && (uint32_t)idx[h] <= thri);
          code = kp ? 1 : 0;
        }
        if (keep_of(ga)) keep_of(ga)[idx[h]] = code;
        nkept += kp ? 1u : 0u;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          s[r] += kp ? p[h][r] : 0.0;
          s[3 + r] += kp ? y[r] : 0.0;
#pragma unroll
          for (int c = 0; c < 3; c++) s[6 + 3 * r + c] += kp ? p[h][r] * y[c] : 0.0;
        }
        s[15] += kp ? dd : 0.0;
        if constexpr (SIM) {
          s[16] += kp ? (p[h][0] * p[h][0] + p[h][1] * p[h][1]) + p[h][2] * p[h][2] : 0.0;
          s[17] += kp ? (y0 * y0 + y1 * y1) + y2 * y2 : 0.0;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 3; r++) {
          s[r] += p[h][r];
          s[3 + r] += y[r];
#pragma unroll
          for (int c = 0; c < 3; c++) s[6 + 3 * r + c] += p[h][r] * y[c];
        }
        const double e0 = p[h][0] - y0, e1 = p[h][1] - y1, e2 = p[h][2] - y2;
        s[15] += e0 * e0 + e1 * e1 + e2 * e2;
      }
    }
  }
  if constexpr (!DIST) block_fold<TB>(s, FoldSum(), partial + (size_t)blockIdx.x * NS);
  if constexpr (GATED || RSUM) block_count<TB>(nkept, pkept_of(ga) + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
  if constexpr (USUM) {
    __syncthreads();  // block_count's LDS words are free again
    block_count<TB>(nlost, ga.a.plost + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
  }
}

template <int TB>
__global__ __launch_bounds__(TB) void k_icp_pass_small(const double* __restrict__ model, const float4* __restrict__ model32,
                                                      int nm, const double* __restrict__ data, int64_t nd,
                                                      const IcpState* __restrict__ st, double* __restrict__ partial,
                                                      int32_t* __restrict__ nn, uint32_t imask, double tolk) {
  icp_pass_small_body<TB>(model, model32, nm, data, nd, st, partial, nn, imask, tolk, NoGate());
}
template <int TB>
__global__ __launch_bounds__(TB) void k_icp_pass_small_gated(const double* __restrict__ model,
                                                            const float4* __restrict__ model32, int nm,
                                                            const double* __restrict__ data, int64_t nd,
                                                            const IcpState* __restrict__ st, double* __restrict__ partial,
                                                            int32_t* __restrict__ nn, uint32_t imask, double tolk,
                                                            GateArgs ga) {
  icp_pass_small_body<TB>(model, model32, nm, data, nd, st, partial, nn, imask, tolk, ga);
}

template <int TB>
__global__ __launch_bounds__(TB) void k_icp_pass_small_sim(const double* __restrict__ model,
                                                          const float4* __restrict__ model32, int nm,
                                                          const double* __restrict__ data, int64_t nd,
                                                          const IcpState* __restrict__ st, double* __restrict__ partial,
                                                          int32_t* __restrict__ nn, uint32_t imask, double tolk,
                                                          SimGate ga) {
  icp_pass_small_body<TB>(model, model32, nm, data, nd, st, partial, nn, imask, tolk, ga);
}

// The trimmed round's two passes (G = TrimDist, TrimSum): the same bodies, partition and fold.
template <int TB, int NNMODE, class G>
__global__ __launch_bounds__(TB) void k_icp_pass_trim(const double* __restrict__ model,
                                                     const float4* __restrict__ model32, int nm,
                                                     const double* __restrict__ data, int64_t nd,
                                                     const IcpState* __restrict__ st, double* __restrict__ partial,
                                                     NNGrid ng, G ta) {
  icp_pass_body<TB, NNMODE>(model, model32, nm, data, nd, st, partial, nullptr, ng, ta);
}
template <int TB, class G>
__global__ __launch_bounds__(TB) void k_icp_pass_small_trim(const double* __restrict__ model,
                                                           const float4* __restrict__ model32, int nm,
                                                           const double* __restrict__ data, int64_t nd,
                                                           const IcpState* __restrict__ st, double* __restrict__ partial,
                                                           uint32_t imask, double tolk, G ta) {
  icp_pass_small_body<TB>(model, model32, nm, data, nd, st, partial, nullptr, imask, tolk, ta);
}

// The unique-correspondence round's two passes (G = UniqDist, UniqSum): the same bodies, partition and fold.
template <int TB, int NNMODE, class G>
__global__ __launch_bounds__(TB) void k_icp_pass_uniq(const double* __restrict__ model,
                                                     const float4* __restrict__ model32, int nm,
                                                     const double* __restrict__ data, int64_t nd,
                                                     const IcpState* __restrict__ st, double* __restrict__ partial,
                                                     NNGrid ng, G ua) {
  icp_pass_body<TB, NNMODE>(model, model32, nm, data, nd, st, partial, nullptr, ng, ua);
}
template <int TB, class G>
__global__ __launch_bounds__(TB) void k_icp_pass_small_uniq(const double* __restrict__ model,
                                                           const float4* __restrict__ model32, int nm,
                                                           const double* __restrict__ data, int64_t nd,
                                                           const IcpState* __restrict__ st, double* __restrict__ partial,
                                                           uint32_t imask, double tolk, G ua) {
  icp_pass_small_body<TB>(model, model32, nm, data, nd, st, partial, nullptr, imask, tolk, ua);
}

// ---- the tie pass and the slot reset of a unique-correspondence round -----------------------------------------------
// After the distance pass a slot's key is the smallest K(dd) among the landmarks on that target.  Every landmark whose
// K equals it takes the minimum of its index in the slot's second word: the slot then names the smallest 96-bit key.
// Integer atomics alone: the result is the same in any order of execution.  grid (workgroups over L, poses).
__global__ __launch_bounds__(ITPB) void k_icpu_tie(const IcpState* __restrict__ st, UniqArgs a, int64_t L) {
  const int h = blockIdx.y;
  if (st[h].done) return;
  const unsigned long long* key = a.key + (size_t)h * (size_t)L;
  const int32_t* nn = a.nn + (size_t)h * (size_t)L;
  const unsigned long long* skey = a.skey + (size_t)h * (size_t)a.nt;
  uint32_t* sidx = a.sidx + (size_t)h * (size_t)a.nt;
  for (int64_t i = (int64_t)blockIdx.x * ITPB + threadIdx.x; i < L; i += (int64_t)gridDim.x * ITPB) {
    const int32_t j = nn[i];
    if (key[i] == skey[j]) atomicMin(&sidx[j], (uint32_t)i);
  }
}
// The slots a round's landmarks touched, all ones again: L stores per pose through the stored nn, whatever nt.  The
// step of a round does it for up to UNIQ_RESET_STEP_MAX landmarks; beyond, k_icpu_reset runs between the sums pass and
// the step over many workgroups (same grid as k_icpu_tie).
constexpr int UNIQ_RESET_STEP_MAX = 4096;
constexpr int UNIQ_TIE_KEYS = 2048;  // landmarks per workgroup of k_icpu_tie / k_icpu_reset, up to UNIQ_TIE_BLOCKS per pose
constexpr int UNIQ_TIE_BLOCKS = 256;
__device__ __forceinline__ void uniq_reset(const UniqArgs& a, int h, int64_t L, int64_t first, int64_t stride) {
  const int32_t* nn = a.nn + (size_t)h * (size_t)L;
  unsigned long long* skey = a.skey + (size_t)h * (size_t)a.nt;
  uint32_t* sidx = a.sidx + (size_t)h * (size_t)a.nt;
  for (int64_t i = first; i < L; i += stride) {
    const int32_t j = nn[i];
    skey[j] = ~0ull;
    sidx[j] = ~0u;
  }
}
__global__ __launch_bounds__(ITPB) void k_icpu_reset(const IcpState* __restrict__ st, UniqArgs a, int64_t L) {
  const int h = blockIdx.y;
  if (st[h].done) return;
  uniq_reset(a, h, L, (int64_t)blockIdx.x * ITPB + threadIdx.x, (int64_t)gridDim.x * ITPB);
}

// ---- the select of a trimmed round ------------------------------------------------------------------------------
// Rank m (1-based) over the L distinct 96-bit strings [K(dd) | landmark], most significant digit first, 8 bits a digit:
// per digit a 256-bin histogram of the strings that agree with the digits chosen so far, then the bin the rank falls
// into.  Only integer compares and integer atomics decide, so the result is the same in any order of execution.
// Up to TRIM_SELECT_WG_MAX landmarks one workgroup per pose stages the keys in LDS and runs all twelve digits
// (k_icpt_select_wg: one launch); beyond, k_icpt_hist runs once per digit over all workgroups with global histograms
// and k_icpt_select_fin closes the round (13 launches, whatever the data).
constexpr int TRIM_SELECT_WG_MAX = VCP_ICPT_SELECT_WG_MAX;  // 4096: 32 KB of keys in LDS
constexpr int TRIM_DIGITS = 12;
constexpr int TRIM_HIST_KEYS = 2048;    // keys per workgroup of k_icpt_hist, up to TRIM_HIST_BLOCKS workgroups per pose
constexpr int TRIM_HIST_BLOCKS = 256;
static_assert(ITPB == 256, "one thread per histogram bin");

struct TrimPrefix {
  uint32_t w0, w1, w2;  // the string's three words (K high, K low, landmark), the digits not chosen yet zero
  uint32_t rank;  // the rank left among the strings that agree with them
};
__device__ __forceinline__ uint32_t trim_word(unsigned long long k, uint32_t i, int w) {
  return w == 0 ? (uint32_t)(k >> 32) : w == 1 ? (uint32_t)k : i;
}
__device__ __forceinline__ uint32_t trim_digit(unsigned long long k, uint32_t i, int d) {
  return (trim_word(k, i, d >> 2) >> (24 - 8 * (d & 3))) & 255u;
}
// whether (k, i) agrees with p in its first d digits
__device__ __forceinline__ bool trim_match(unsigned long long k, uint32_t i, const TrimPrefix& p, int d) {
  // per word: the mask of the bits that lie within the first d digits (named words: an index would go to scratch)
  const int w = d >> 2, b = d & 3;
  const uint32_t part = b ? ~0u << (32 - 8 * b) : 0u;
  const uint32_t m0 = w > 0 ? ~0u : part, m1 = w > 1 ? ~0u : w == 1 ? part : 0u, m2 = w == 2 ? part : 0u;
  return ((((uint32_t)(k >> 32) ^ p.w0) & m0) | (((uint32_t)k ^ p.w1) & m1) | ((i ^ p.w2) & m2)) == 0;
}
__device__ __forceinline__ void trim_push(TrimPrefix& p, int d, uint32_t g, uint32_t rank) {
  const uint32_t add = g << (24 - 8 * (d & 3));
  const int w = d >> 2;
  p.w0 |= w == 0 ? add : 0u;
  p.w1 |= w == 1 ? add : 0u;
  p.w2 |= w == 2 ? add : 0u;
  p.rank = rank;
}
// Thread t holds the count c of bin t; rank r, 1 <= r <= the total: the bin g with below(g) < r <= below(g) + c(g) and
// the rank left in it, to every thread.  sh: 8 words of LDS, free again on return.
__device__ __forceinline__ void trim_pick(uint32_t c, uint32_t r, uint32_t* sh, uint32_t& g, uint32_t& left) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (threadIdx.x == 0) {
    sh[4] = 0;
    sh[5] = 1;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  for (int u = 0; u < w; u++) inc += sh[u];
  const uint32_t exc = inc - c;
  if (exc < r && r <= inc) {
    sh[4] = threadIdx.x;
    sh[5] = r - exc;
  }
  __syncthreads();
  g = sh[4];
  left = sh[5];
  __syncthreads();
}

__global__ __launch_bounds__(ITPB) void k_icpt_select_wg(const IcpState* __restrict__ st, TrimArgs a, int L) {
  const int h = blockIdx.x;
  st += h;
  if (st->done) return;
  __shared__ unsigned long long sk[TRIM_SELECT_WG_MAX];
  __shared__ uint32_t hist[ITPB], sh[8];
  const unsigned long long* key = a.key + (size_t)h * L;
  for (int i = threadIdx.x; i < L; i += ITPB) sk[i] = key[i];
  TrimPrefix p{0u, 0u, 0u, (uint32_t)trim_m(a, st, L)};
  for (int d = 0; d < TRIM_DIGITS; d++) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += ITPB) {
      const unsigned long long k = sk[i];
      if (trim_match(k, (uint32_t)i, p, d)) atomicAdd(&hist[trim_digit(k, (uint32_t)i, d)], 1u);
    }
    __syncthreads();
    uint32_t g, left;
    trim_pick(hist[threadIdx.x], p.rank, sh, g, left);
    trim_push(p, d, g, left);
  }
  if (threadIdx.x == 0) a.sel[h] = TrimSel{((unsigned long long)p.w0 << 32) | p.w1, p.w2, 0u};
}

// digit d of the multi-workgroup form: ghist [poses][12][256], zero on entry of a round; slot [poses][12], slot d = the
// prefix and rank before digit d (written by workgroup 0 of this launch, read by the next)
__global__ __launch_bounds__(ITPB) void k_icpt_hist(const IcpState* __restrict__ st, TrimArgs a, int64_t L,
                                                   uint32_t* __restrict__ ghist, TrimPrefix* __restrict__ slot, int d) {
  const int h = blockIdx.y;
  st += h;
  if (st->done) return;
  __shared__ uint32_t hist[ITPB], sh[8];
  ghist += (size_t)h * TRIM_DIGITS * ITPB;
  slot += (size_t)h * TRIM_DIGITS;
  TrimPrefix p{0u, 0u, 0u, 0u};
  if (d == 0) {
    p.rank = (uint32_t)trim_m(a, st, L);
  } else {
    p = slot[d - 1];
    uint32_t g, left;
    trim_pick(ghist[(d - 1) * ITPB + threadIdx.x], p.rank, sh, g, left);
    trim_push(p, d - 1, g, left);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) slot[d] = p;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long* key = a.key + (size_t)h * (size_t)L;
  for (int64_t i = (int64_t)blockIdx.x * ITPB + threadIdx.x; i < L; i += (int64_t)gridDim.x * ITPB) {
    const unsigned long long k = key[i];
    if (trim_match(k, (uint32_t)i, p, d)) atomicAdd(&hist[trim_digit(k, (uint32_t)i, d)], 1u);
  }
  __syncthreads();
  const uint32_t c = hist[threadIdx.x];
  if (c) atomicAdd(&ghist[d * ITPB + threadIdx.x], c);
}

// the last digit's bin, the selected string into sel, and the histograms zero again for the next round
__global__ __launch_bounds__(ITPB) void k_icpt_select_fin(const IcpState* __restrict__ st, TrimArgs a,
                                                         uint32_t* __restrict__ ghist,
                                                         const TrimPrefix* __restrict__ slot) {
  const int h = blockIdx.x;
  st += h;
  if (st->done) return;
  __shared__ uint32_t sh[8];
  ghist += (size_t)h * TRIM_DIGITS * ITPB;
  TrimPrefix p = slot[(size_t)h * TRIM_DIGITS + TRIM_DIGITS - 1];
  uint32_t g, left;
  trim_pick(ghist[(TRIM_DIGITS - 1) * ITPB + threadIdx.x], p.rank, sh, g, left);
  trim_push(p, TRIM_DIGITS - 1, g, left);
  if (threadIdx.x == 0) a.sel[h] = TrimSel{((unsigned long long)p.w0 << 32) | p.w1, p.w2, 0u};
  for (int d = 0; d < TRIM_DIGITS; d++) ghist[d * ITPB + threadIdx.x] = 0;
}

// ---- Horn's unit-quaternion closed form (host and device: same code, same rounding) -----------------
// cyclic Jacobi sweeps on a symmetric 4x4 (independent of the oracle's max-pivot variant).  Every index is a
// compile-time constant after unrolling, so on the device A and V live in registers (dynamic indexing would put
// them in scratch memory and make the single solving thread several times slower).
template <int P, int Q>
__host__ __device__ inline void jrot(double (&A)[4][4], double (&V)[4][4]) {
  if (A[P][Q] == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * A[P][Q]);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// A = V0^T Q V0 and V = V0 on entry (V0 = identity for a cold start): on return the columns of V are eigenvectors of Q
__host__ __device__ inline void jacobi4(double (&A)[4][4], double (&V)[4][4]) {
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      diag += A[i][i] * A[i][i];
#pragma unroll
      for (int j = i + 1; j < 4; j++) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-34 * (diag + off) || off == 0.0) break;
    // three rounds of two rotations in DISJOINT planes: the angle of the second reads nothing the first one writes, so
    // the two chains of divisions and square roots overlap in the single lane that runs this
    jrot<0, 1>(A, V);
    jrot<2, 3>(A, V);
    jrot<0, 2>(A, V);
    jrot<1, 3>(A, V);
    jrot<0, 3>(A, V);
    jrot<1, 2>(A, V);
  }
}

// Vst [16]: the eigenvector basis of the previous round (row major), or NULL.  Consecutive rounds of an ICP solve
// nearly the same 4x4 problem, so the sweeps start from the previous basis (A = V^T Q V is then almost diagonal: one
// or two sweeps instead of six or seven -- the Jacobi chain is what bounds k_icp_step); the basis found is stored back.
// A basis that is not finite or has drifted from orthonormal (first round, failed round) is replaced by the identity.
__host__ __device__ inline bool horn(const double s[16], long long nd, double R1[9], double T1[3], double* Vst) {
  const double N = (double)nd;
  double Q[4][4], V[4][4];
  if (Vst) {  // read first: on the device the loads then fly while the divisions below run
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) V[i][j] = Vst[4 * i + j];
  }
  double muP[3], muY[3], m[3][3];
  for (int a = 0; a < 3; a++) {
    muP[a] = s[a] / N;
    muY[a] = s[3 + a] / N;
  }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) m[r][c] = s[6 + 3 * r + c] / N - muP[r] * muY[c];
  const double tr = m[0][0] + m[1][1] + m[2][2];
  const double delta[3] = {m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]};
  Q[0][0] = tr;
  for (int i = 0; i < 3; i++) {
    Q[0][i + 1] = Q[i + 1][0] = delta[i];
    for (int j = 0; j < 3; j++) Q[i + 1][j + 1] = m[i][j] + m[j][i] - (i == j ? tr : 0.0);
  }
  // Q goes into the sweeps divided by the power of two that brings its largest entry into [0.5, 1): jacobi4's stop test
  // squares the entries, and beyond about 2^+-256 the squares overflow or flush to zero, which ended the sweeps before
  // the first rotation with "solved".  The division is exact and R1 depends on the eigenvectors alone, so nothing
  // changes where the squares were in range.  A non-finite entry (non-finite sums, or sums that overflow here) fails the
  // solve: an infinite off-diagonal entry passed the same stop test.  Tested per entry: fmax would drop a NaN.  The
  // verdict is returned at the end, not here: a branch at this point keeps the device compiler from issuing the loads
  // of the basis early, and the failing case may take as long as it likes.
  double rmax[4];  // per row of the upper triangle: four short chains instead of one of ten
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    rmax[i] = 0.0;
#pragma unroll
    for (int j = i; j < 4; j++) {
      const double a = fabs(Q[i][j]);
      finite = finite && (a <= 1.7976931348623157e308);  // false for NaN
      rmax[i] = a > rmax[i] ? a : rmax[i];
    }
  }
  const double m01 = rmax[0] > rmax[1] ? rmax[0] : rmax[1], m23 = rmax[2] > rmax[3] ? rmax[2] : rmax[3];
  const double qmax = finite ? (m01 > m23 ? m01 : m23) : 0.0;
  int e;  // 0 for qmax = 0 (coincident points, or a Q that fails anyway)
  (void)frexp(qmax, &e);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) Q[i][j] = ldexp(Q[i][j], -e);
  bool warm = Vst != nullptr;
  if (warm) {
    bool ortho = true;  // | V^T V - I |_max <= 1e-9, tested per entry: fmax would drop a NaN
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = i; j < 4; j++) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) d += V[k][i] * V[k][j];
        ortho = ortho && (fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-9);  // false for NaN
      }
    warm = ortho;
  }
  if (warm) {
    double QV[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) d += Q[i][k] * V[k][j];
        QV[i][j] = d;
      }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = i; j < 4; j++) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) d += V[k][i] * QV[k][j];
        Q[i][j] = d;
        Q[j][i] = d;
      }
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  }
  jacobi4(Q, V);
  if (Vst) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) Vst[4 * i + j] = V[i][j];
  }
  // eigenvector of the largest eigenvalue, picked without dynamic indexing (first maximum wins)
  double ev = Q[0][0];
  double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int i = 1; i < 4; i++)
    if (Q[i][i] > ev) {
      ev = Q[i][i];
#pragma unroll
      for (int k = 0; k < 4; k++) q[k] = V[k][i];
    }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!finite || !(nrm > 0.0) || !(nrm <= 1.7976931348623157e308)) return false;
  for (int i = 0; i < 4; i++) q[i] /= nrm;
  // CalculateRotation, BaseClass/ICP.cs:274-285
  R1[0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3];
  R1[1] = 2.0 * (q[1] * q[2] - q[0] * q[3]);
  R1[2] = 2.0 * (q[1] * q[3] + q[0] * q[2]);
  R1[3] = 2.0 * (q[1] * q[2] + q[0] * q[3]);
  R1[4] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3];
  R1[5] = 2.0 * (q[2] * q[3] - q[0] * q[1]);
  R1[6] = 2.0 * (q[1] * q[3] - q[0] * q[2]);
  R1[7] = 2.0 * (q[2] * q[3] + q[0] * q[1]);
  R1[8] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
  for (int i = 0; i < 3; i++)
    T1[i] = muY[i] - (R1[3 * i] * muP[0] + R1[3 * i + 1] * muP[1] + R1[3 * i + 2] * muP[2]);
  return true;
}

// The similarity step (vcp.h, "similarity ICP"): horn() on s[0..15] unchanged, then Horn's symmetric scale from the two
// further columns, k = sqrt(vY / vP) with v = sum |x|^2 / N - |mu|^2, which does not depend on the rotation.  c is the
// product of the factors applied so far; the new product c k is held in [ratio_min, ratio_max] by shortening this
// round's factor.  Returns 0 (horn failed: nothing written), 1, or 2 (scale not determined: the rigid step, c stays).
// Every operation is one binary64 rounding; where k_used is 1.0, R1s and T1 are horn()'s bit for bit (1.0 * x = x and
// T1 is horn's expression).
__host__ __device__ inline int horn_sim(const double s[18], long long n, double c, double ratio_min, double ratio_max,
                                        double R1s[9], double T1[3], double* Vst, double* k_used, double* c_new) {
  double R1[9], T1r[3];
  if (!horn(s, n, R1, T1r, Vst)) return 0;
  const double N = (double)n;
  const double muP0 = s[0] / N, muP1 = s[1] / N, muP2 = s[2] / N;  // horn's means: the same divisions
  const double muY0 = s[3] / N, muY1 = s[4] / N, muY2 = s[5] / N;
  const double vP = s[16] / N - ((muP0 * muP0 + muP1 * muP1) + muP2 * muP2);
  const double vY = s[17] / N - ((muY0 * muY0 + muY1 * muY1) + muY2 * muY2);
  const double big = 1.7976931348623157e308;
  const bool det = vP > 0.0 && vP <= big && vY > 0.0 && vY <= big;  // false for NaN
  double ku = 1.0, cn = c;
  if (det) {
    const double k = sqrt(vY / vP), t = c * k;
    if (t < ratio_min) {
      cn = ratio_min;
      ku = ratio_min / c;
    } else if (t > ratio_max) {
      cn = ratio_max;
      ku = ratio_max / c;
    } else {
      cn = t;
      ku = k;
    }
  }
#pragma unroll
  for (int j = 0; j < 9; j++) R1s[j] = ku * R1[j];
  const double muY[3] = {muY0, muY1, muY2};
#pragma unroll
  for (int i = 0; i < 3; i++) T1[i] = muY[i] - (R1s[3 * i] * muP0 + R1s[3 * i + 1] * muP1 + R1s[3 * i + 2] * muP2);
  *k_used = ku;
  *c_new = cn;
  return det ? 1 : 2;
}

// R <- R1 R, T <- R1 T + T1 in the state (BaseClass/ICP.cs:163-177)
__device__ __forceinline__ void icp_compose(IcpState* __restrict__ st, const double R1[9], const double T1[3]) {
  double tR[9], tT[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double acc = 0.0;
      for (int k = 0; k < 3; k++) acc += R1[3 * i + k] * st->R[3 * k + j];
      tR[3 * i + j] = acc;
    }
  for (int i = 0; i < 3; i++) {
    double acc = 0.0;
    for (int k = 0; k < 3; k++) acc += R1[3 * i + k] * st->T[k];
    tT[i] = acc + T1[i];
  }
  for (int k = 0; k < 9; k++) st->R[k] = tR[k];
  for (int k = 0; k < 3; k++) st->T[k] = tT[k];
}

// What follows the pass: fixed-order reduction of the partial rows (thread t adds rows t, t+TB, ... in order, then a
// fixed shuffle/LDS tree: bitwise reproducible, no float atomics), then thread 0 advances the ICP state by one round.
// (Running this in the pass's last workgroup -- ticket + release fence per workgroup -- was built and measured at
// 1 M x 100: 74 us per round against 51 us for the two launches; the Horn solve's registers also halve the pass's
// occupancy.  It stays a launch of its own.)
// NS: columns of a row (18: the similarity pass; the state holds the first 16 all the same).
template <int TB, int NS = 16>
__device__ __forceinline__ void icp_fold_rows(const double* __restrict__ partial, int nb, IcpState* __restrict__ st,
                                              double* tot) {
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) s[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += TB) {
#pragma unroll
    for (int k = 0; k < NS; k++)
      s[k] += partial[(size_t)b * NS + k];
  }
  block_fold<TB>(s, FoldSum(), tot);
  if (threadIdx.x < 16) st->sums[threadIdx.x] = tot[threadIdx.x];
  __syncthreads();
}

template <int TB>
__device__ __forceinline__ void icp_step_body(const double* __restrict__ partial, int nb, IcpState* __restrict__ st,
                                              const StepArgs& a) {
  __shared__ double tot[16];
  icp_fold_rows<TB>(partial, nb, st, tot);
  if (threadIdx.x != 0) return;
  if (a.mode == MODE_SUMS_ONLY) {
    st->done = 1;
    return;
  }
  double S[16];
  for (int k = 0; k < 16; k++) S[k] = tot[k];
  double R1[9], T1[3];
  const bool ok = horn(S, a.nd, R1, T1, st->V);
  const double pre_d = st->d;
  const double d = S[15];
  st->pre_d = pre_d;
  st->d = d;
  const int round = st->round + 1;
  st->round = round;
  bool go;
  if (a.mode == MODE_VTK) go = true;  // fixed number of rounds, mean-distance check off (FrmMain.cs:855-858)
  else if (a.stop_rule == VCP_STOP_RMSE) go = sqrt(d / (double)a.nd) >= a.tol;
  else go = fabs(d - pre_d) >= a.tol;  // BaseClass/ICP.cs:149,180
  if (go) {
    if (!ok) {
      st->failed = 1;
      st->done = 1;
      return;
    }
    if (a.mode == MODE_REFERENCE && round == 1) {  // :151-162 the first result overwrites R, T
      for (int k = 0; k < 9; k++) st->R[k] = R1[k];
      for (int k = 0; k < 3; k++) st->T[k] = T1[k];
    } else {  // :163-177  R <- R1 R, T <- R1 T + T1
      icp_compose(st, R1, T1);
    }
  }
  if (!go || round >= a.max_iter) st->done = 1;
}

// one workgroup per state: blockIdx.x selects the state and its nb partial rows
__global__ __launch_bounds__(ITPB) void k_icp_step(const double* __restrict__ partial, int nb, IcpState* __restrict__ st,
                                                  StepArgs a) {
  st += blockIdx.x;
  partial += (size_t)blockIdx.x * nb * 16;
  if (st->done) return;
  icp_step_body<ITPB>(partial, nb, st, a);
}

// The step of a gated round (vcp.h, vcp_icp_gated): the same fold of the partial rows, the kept counts of the
// workgroups added up (integers: exact), then Horn on (sums, kept) and the composition -- or, with fewer than
// min_pairs pairs kept, nothing: R, T and the basis V stay, the round counts and `starved` goes up.  Always max_iter
// rounds, as MODE_VTK.  sums_only: the pass alone (vcp_icp_sums_gated).
struct GateStepArgs {
  long long min_pairs;
  int max_iter, sums_only;
};
__global__ __launch_bounds__(ITPB) void k_icp_step_gated(const double* __restrict__ partial,
                                                        const uint32_t* __restrict__ pkept, int nb,
                                                        IcpState* __restrict__ st, GateStepArgs a) {
  st += blockIdx.x;
  partial += (size_t)blockIdx.x * nb * 16;
  pkept += (size_t)blockIdx.x * nb;
  if (st->done) return;
  __shared__ double tot[16];
  __shared__ unsigned long long skept;
  if (threadIdx.x == 0) skept = 0;
  icp_fold_rows<ITPB>(partial, nb, st, tot);  // its barrier orders the store above before the adds below
  unsigned long long c = 0;
  for (int b = threadIdx.x; b < nb; b += ITPB) c += pkept[b];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&skept, c);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long kept = (long long)skept;
  st->kept = kept;
  if (a.sums_only) {
    st->done = 1;
    return;
  }
  st->pre_d = st->d;
  st->d = tot[15];
  const int round = st->round + 1;
  st->round = round;
  if (kept < a.min_pairs) {
    st->starved = st->starved + 1;
  } else {
    double S[16];
    for (int k = 0; k < 16; k++) S[k] = tot[k];
    double R1[9], T1[3];
    if (!horn(S, kept, R1, T1, st->V)) {
      st->failed = 1;
      st->done = 1;
      return;
    }
    icp_compose(st, R1, T1);
  }
  if (round >= a.max_iter) st->done = 1;
}

// The step of a unique-correspondence round (vcp.h, vcp_icp_unique): k_icp_step_gated, word for word, on the sums
// pass's rows and kept counts; beside it the lost counts of the workgroups added up into the pose's side record (the
// state has no room for it), and -- reset_L > 0 -- the round's slots set back to all ones (uniq_reset).
__global__ __launch_bounds__(ITPB) void k_icp_step_unique(const double* __restrict__ partial, int nb,
                                                         IcpState* __restrict__ st, long long* __restrict__ lost,
                                                         UniqArgs ua, long long reset_L, GateStepArgs a) {
  const int h = blockIdx.x;
  st += h;
  partial += (size_t)h * nb * 16;
  const uint32_t* pkept = ua.pkept + (size_t)h * nb;
  const uint32_t* plost = ua.plost + (size_t)h * nb;
  if (st->done) return;
  __shared__ double tot[16];
  __shared__ unsigned long long skept, slost;
  if (threadIdx.x == 0) {
    skept = 0;
    slost = 0;
  }
  icp_fold_rows<ITPB>(partial, nb, st, tot);  // its barrier orders the stores above before the adds below
  unsigned long long c = 0, l = 0;
  for (int b = threadIdx.x; b < nb; b += ITPB) {
    c += pkept[b];
    l += plost[b];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    c += __shfl_down(c, d, 64);
    l += __shfl_down(l, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&skept, c);
    atomicAdd(&slost, l);
  }
  if (reset_L > 0) uniq_reset(ua, h, reset_L, threadIdx.x, ITPB);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long kept = (long long)skept;
  st->kept = kept;
  lost[h] = (long long)slost;
  if (a.sums_only) {
    st->done = 1;
    return;
  }
  st->pre_d = st->d;
  st->d = tot[15];
  const int round = st->round + 1;
  st->round = round;
  if (kept < a.min_pairs) {
    st->starved = st->starved + 1;
  } else {
    double S[16];
    for (int k = 0; k < 16; k++) S[k] = tot[k];
    double R1[9], T1[3];
    if (!horn(S, kept, R1, T1, st->V)) {
      st->failed = 1;
      st->done = 1;
      return;
    }
    icp_compose(st, R1, T1);
  }
  if (round >= a.max_iter) st->done = 1;
}

// The step of a similarity round (vcp.h, vcp_icp_sim): k_icp_step_gated over 18-wide rows, with horn_sim in horn's
// place.  What the state has no room for lives in the pose's side record: the two further sums, the product c of the
// factors applied and the count of rounds whose scale was not determined.
struct SimSide {
  double s16, s17;  // the last pass's sums[16], sums[17]
  double c;
  int unscaled, pad;
};
struct SimStepArgs {
  double ratio_min, ratio_max;
};
__global__ __launch_bounds__(ITPB) void k_icp_step_sim(const double* __restrict__ partial,
                                                      const uint32_t* __restrict__ pkept, int nb,
                                                      IcpState* __restrict__ st, SimSide* __restrict__ side,
                                                      GateStepArgs a, SimStepArgs sa) {
  st += blockIdx.x;
  side += blockIdx.x;
  partial += (size_t)blockIdx.x * nb * 18;
  pkept += (size_t)blockIdx.x * nb;
  if (st->done) return;
  __shared__ double tot[18];
  __shared__ unsigned long long skept;
  if (threadIdx.x == 0) skept = 0;
  icp_fold_rows<ITPB, 18>(partial, nb, st, tot);  // its barrier orders the store above before the adds below
  unsigned long long c = 0;
  for (int b = threadIdx.x; b < nb; b += ITPB) c += pkept[b];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&skept, c);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long kept = (long long)skept;
  st->kept = kept;
  side->s16 = tot[16];
  side->s17 = tot[17];
  if (a.sums_only) {
    st->done = 1;
    return;
  }
  st->pre_d = st->d;
  st->d = tot[15];
  const int round = st->round + 1;
  st->round = round;
  if (kept < a.min_pairs) {
    st->starved = st->starved + 1;
  } else {
    double S[18];
    for (int k = 0; k < 18; k++) S[k] = tot[k];
    double R1s[9], T1[3], ku, cn;
    const int rc = horn_sim(S, kept, side->c, sa.ratio_min, sa.ratio_max, R1s, T1, st->V, &ku, &cn);
    if (rc == 0) {
      st->failed = 1;
      st->done = 1;
      return;
    }
    side->c = cn;
    if (rc == 2) side->unscaled = side->unscaled + 1;
    icp_compose(st, R1s, T1);
  }
  if (round >= a.max_iter) st->done = 1;
}

void identity(IcpState& s) {
  std::memset(&s, 0, sizeof(s));
  s.R[0] = s.R[4] = s.R[8] = 1.0;
}

// device layout of b_icp_part: the states first, the partial rows from the next 256-byte boundary
size_t icp_states_bytes(int nst) { return ((size_t)nst * sizeof(IcpState) + 255) & ~(size_t)255; }
IcpState* icp_states(vcp_ctx* ctx) { return ctx->b_icp_part.as<IcpState>(); }

// Runs rounds on device-resident model/data until the states say done.  `init` carries the starting R,T of nst
// independent states (nst > 1: vcp_icp_multistart, MODE_VTK), `out` receives them.  all_rounds: enqueue every round
// and synchronise once (a fixed round count needs nothing back in between).  ng_out (may be NULL) receives the
// model's grid; ng_out->rec == nullptr when the full scans serve the model.
// gr (may be NULL): a gated run -- the gated passes and step, MODE_VTK's fixed round count or MODE_SUMS_ONLY; the
// partition, and with it the tree of the sums, is the ungated one.
struct GateRun {
  const double* gates;  // host, [n_gates], validated by the caller
  int n_gates;
  long long min_pairs;
  uint8_t* d_keep;  // [nd] or NULL
};
// sr (may be NULL; only with gr): the gated run's similarity form -- 18-wide rows, the passes of SimGate and
// k_icp_step_sim; the side records follow the kept counts on the device and the schedule in the staging area.
struct SimRun {
  double ratio_min, ratio_max;  // validated by the caller
  SimSide* side_out;            // host, [nst]
};
// tr (may be NULL; never with gr): a trimmed run -- per round the distance pass, the select, the trimmed sums pass and
// the gated step.  Its workspace is b_icpt: per (pose, landmark) 8 bytes of key and 4 of index, then per pose the
// multi-workgroup select's 12 prefixes and 12 x 256 counters.
struct TrimRun {
  const double* share;  // host, [n_share], validated by the caller; NULL with m_fixed > 0
  int n_share;
  long long m_fixed;
  long long min_pairs;
  uint8_t* d_keep;   // [nd] or NULL
  TrimSel* sel_out;  // host, [nst]: the last select of every pose
};
// ur (may be NULL; never with gr or tr): a unique-correspondence run -- per round the distance pass, the tie pass, the
// sums pass and k_icp_step_unique.  Its workspace is b_icpt too: the trimmed run's 12 bytes per (pose, landmark), then
// the slots, 8 bytes of key per (pose, target) and then 4 of index, all ones from one fill per call and from the reset
// of every round.
struct UniqRun {
  const double* gates;  // host, [n_gates], validated by the caller
  int n_gates;
  long long min_pairs;
  uint8_t* d_keep;      // [nd] or NULL
  long long* lost_out;  // host, [nst]: the last round's count of every pose
};
size_t icpt_keys_bytes(int nst, int64_t nd) { return ((size_t)nst * (size_t)nd * 12 + 255) & ~(size_t)255; }
int32_t* icpt_nn(vcp_ctx* ctx, int nst, int64_t nd) {
  return reinterpret_cast<int32_t*>(ctx->b_icpt.as<char>() + (size_t)nst * (size_t)nd * 8);
}
int icp_run(vcp_ctx* ctx, const double* d_model, int64_t nm, const double* d_data, int64_t nd, const IcpState* init,
            int nst, double tol, int stop_rule, int max_iter, int mode, IcpState* out, int32_t* d_nn, bool all_rounds,
            NNGrid* ng_out, const GateRun* gr = nullptr, const TrimRun* tr = nullptr, const SimRun* sr = nullptr,
            const UniqRun* ur = nullptr) {
  hipStream_t st = ctx->stream;
  // small data sets: one wave per workgroup so that they reach more CUs; large models: LDS tiles
  const bool small0 = nd <= (int64_t)64 * ICP_MAX_BLOCKS;
  // models beyond the scalar cache: binned once per call (they do not move), grid search per data point; a model with
  // non-finite coordinates keeps the LDS-tiled full scan
  NNGrid ng{};
  bool grid = false;
  if (nm > 512) {
    const int grc = vcp_nngrid_build(ctx, d_model, nm, &ng);
    if (grc == VCP_OK) grid = true;
    else if (grc != VCP_ERR_UNSUPPORTED) return grc;
  }
  if (ng_out) *ng_out = ng;
  const bool tiled = nm > 512 && !grid;
  const bool small = grid ? nd * nng::NNG <= (int64_t)64 * ICP_MAX_BLOCKS : small0;
  const int tb = small ? 64 : ITPB;
  const bool pairs = !grid && !tiled;  // scalar-cache models: two data points per lane (k_icp_pass_small)
  // tb, nb and the path fix the order of the 16 sums bit for bit: restated as plan() in tests/icp_sums_ref.py, change both
  const int nb = (int)vcp_blocks(grid ? nd * nng::NNG : pairs ? (nd + 1) / 2 : nd, tb, ICP_MAX_BLOCKS);
  int ib = 1;
  while ((1 << ib) < (int)nm) ib++;
  const uint32_t imask = (1u << ib) - 1u;
  double tolk = 1.0;  // smallest power of two >= (54 + 9 * 2^ib) * 2^-24
  while (tolk * 0.5 >= (54.0 + 9.0 * (double)(1u << ib)) / 16777216.0) tolk *= 0.5;
  // the nst states (icp_states), then [nst][nb][16] partial rows; a gated run: then the schedule and [nst][nb] counts
  const size_t st_bytes = icp_states_bytes(nst);
  const int ncol = sr ? 18 : 16;
  const size_t part_bytes = (size_t)nst * nb * ncol * sizeof(double);
  const int n_sched = gr ? gr->n_gates : tr ? tr->n_share : ur ? ur->n_gates : 0;  // doubles staged behind the partial rows
  const size_t cnt_bytes = ((size_t)nst * nb * sizeof(uint32_t) + 15) & ~(size_t)15;
  const size_t side_bytes = sr ? (size_t)nst * sizeof(SimSide) : 0;
  const size_t gate_bytes = gr   ? (size_t)n_sched * sizeof(double) + cnt_bytes + side_bytes
                            : tr ? (size_t)n_sched * sizeof(double) + cnt_bytes + (size_t)nst * sizeof(TrimSel)
                            : ur ? (size_t)n_sched * sizeof(double) + 2 * cnt_bytes + (size_t)nst * sizeof(long long)
                                 : 0;
  VCP_TRY(vcp_ensure(ctx, ctx->b_icp_part, st_bytes + part_bytes + gate_bytes));
  const bool sel_wg = nd <= TRIM_SELECT_WG_MAX;
  const size_t key_bytes = tr || ur ? icpt_keys_bytes(nst, nd) : 0;
  const size_t selws_bytes = (size_t)nst * TRIM_DIGITS * (sizeof(TrimPrefix) + ITPB * sizeof(uint32_t));
  if (tr) VCP_TRY(vcp_ensure(ctx, ctx->b_icpt, key_bytes + selws_bytes));
  const size_t slot_n = ur ? (size_t)nst * (size_t)nm : 0;  // slots: one per (pose, target)
  if (ur) VCP_TRY(vcp_ensure(ctx, ctx->b_icpt, key_bytes + slot_n * 12));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux0, (size_t)nm * sizeof(float4) + 64));
  IcpState* d_st = icp_states(ctx);
  double* part = reinterpret_cast<double*>(ctx->b_icp_part.as<char>() + st_bytes);
  const StepArgs sa{(long long)nd, tol, stop_rule, max_iter, mode};
  float4* model32 = ctx->b_aux0.as<float4>();
  // a gated run stages its schedule behind the states: the caller's array may be gone before the copy has run
  const size_t h_bytes =
      (size_t)nst * sizeof(IcpState) + (size_t)n_sched * sizeof(double) + (tr ? (size_t)nst * sizeof(TrimSel) : 0) +
      (sr ? (size_t)nst * sizeof(SimSide) : 0) + (ur ? (size_t)nst * sizeof(long long) : 0);
  IcpState* h_st = reinterpret_cast<IcpState*>(nst == 1 && !gr && !tr && !ur ? ctx->pinned : vcp_stage(ctx, h_bytes));
  if (!h_st) return vcp_fail(ctx, VCP_ERR_NOMEM, "pinned staging of %d ICP states", nst);
  std::memcpy(h_st, init, (size_t)nst * sizeof(IcpState));
  VCP_HIP(ctx, hipMemcpyAsync(d_st, h_st, (size_t)nst * sizeof(IcpState), hipMemcpyHostToDevice, st));
  GateArgs ga{};
  GateStepArgs gsa{};
  SimGate sga{};
  SimStepArgs ssa{};
  SimSide *d_side = nullptr, *h_side = nullptr;
  if (gr) {
    double* d_gates = reinterpret_cast<double*>(ctx->b_icp_part.as<char>() + st_bytes + part_bytes);
    ga = GateArgs{d_gates, gr->n_gates, reinterpret_cast<uint32_t*>(d_gates + gr->n_gates), gr->d_keep};
    gsa = GateStepArgs{gr->min_pairs, max_iter, mode == MODE_SUMS_ONLY ? 1 : 0};
    double* h_gates = reinterpret_cast<double*>(h_st + nst);
    std::memcpy(h_gates, gr->gates, (size_t)gr->n_gates * sizeof(double));
    VCP_HIP(ctx, hipMemcpyAsync(d_gates, h_gates, (size_t)gr->n_gates * sizeof(double), hipMemcpyHostToDevice, st));
    if (sr) {  // every pose starts at c = 1, no round unscaled
      sga.g = ga;
      ssa = SimStepArgs{sr->ratio_min, sr->ratio_max};
      d_side = reinterpret_cast<SimSide*>(reinterpret_cast<char*>(ga.pkept) + cnt_bytes);
      h_side = reinterpret_cast<SimSide*>(h_gates + gr->n_gates);
      for (int k = 0; k < nst; k++) h_side[k] = SimSide{0.0, 0.0, 1.0, 0, 0};
      VCP_HIP(ctx, hipMemcpyAsync(d_side, h_side, (size_t)nst * sizeof(SimSide), hipMemcpyHostToDevice, st));
    }
  }
  TrimDist td{};
  TrimSum ts{};
  TrimPrefix* d_slot = nullptr;
  uint32_t* d_ghist = nullptr;
  TrimSel* h_sel = nullptr;
  if (tr) {
    double* d_share = reinterpret_cast<double*>(ctx->b_icp_part.as<char>() + st_bytes + part_bytes);
    uint32_t* pkept = reinterpret_cast<uint32_t*>(d_share + n_sched);
    TrimSel* d_sel = reinterpret_cast<TrimSel*>(reinterpret_cast<char*>(pkept) + cnt_bytes);
    td.a = TrimArgs{d_share, n_sched, tr->m_fixed, ctx->b_icpt.as<unsigned long long>(), icpt_nn(ctx, nst, nd),
                    d_sel,   pkept,   tr->d_keep};
    ts.a = td.a;
    gsa = GateStepArgs{tr->min_pairs, max_iter, mode == MODE_SUMS_ONLY ? 1 : 0};
    double* h_share = reinterpret_cast<double*>(h_st + nst);
    h_sel = reinterpret_cast<TrimSel*>(h_share + n_sched);
    if (n_sched) {
      std::memcpy(h_share, tr->share, (size_t)n_sched * sizeof(double));
      VCP_HIP(ctx, hipMemcpyAsync(d_share, h_share, (size_t)n_sched * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // the selects' results are read back at the end; the multi-workgroup form's histograms start at zero
    VCP_HIP(ctx, hipMemsetAsync(d_sel, 0, (size_t)nst * sizeof(TrimSel), st));
    d_slot = reinterpret_cast<TrimPrefix*>(ctx->b_icpt.as<char>() + key_bytes);
    d_ghist = reinterpret_cast<uint32_t*>(d_slot + (size_t)nst * TRIM_DIGITS);
    if (!sel_wg) VCP_HIP(ctx, hipMemsetAsync(d_ghist, 0, (size_t)nst * TRIM_DIGITS * ITPB * sizeof(uint32_t), st));
  }
  UniqDist ud{};
  UniqSum us{};
  long long *d_lost = nullptr, *h_lost = nullptr;
  const bool reset_in_step = nd <= UNIQ_RESET_STEP_MAX;
  if (ur) {
    double* d_gates = reinterpret_cast<double*>(ctx->b_icp_part.as<char>() + st_bytes + part_bytes);
    uint32_t* pkept = reinterpret_cast<uint32_t*>(d_gates + n_sched);
    uint32_t* plost = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(pkept) + cnt_bytes);
    d_lost = reinterpret_cast<long long*>(reinterpret_cast<char*>(plost) + cnt_bytes);
    unsigned long long* skey = reinterpret_cast<unsigned long long*>(ctx->b_icpt.as<char>() + key_bytes);
    ud.a = UniqArgs{d_gates, n_sched, (int)nm, ctx->b_icpt.as<unsigned long long>(), icpt_nn(ctx, nst, nd), skey,
                    reinterpret_cast<uint32_t*>(skey + slot_n), pkept, plost, ur->d_keep};
    us.a = ud.a;
    gsa = GateStepArgs{ur->min_pairs, max_iter, mode == MODE_SUMS_ONLY ? 1 : 0};
    double* h_gates = reinterpret_cast<double*>(h_st + nst);
    h_lost = reinterpret_cast<long long*>(h_gates + n_sched);
    std::memcpy(h_gates, ur->gates, (size_t)n_sched * sizeof(double));
    VCP_HIP(ctx, hipMemcpyAsync(d_gates, h_gates, (size_t)n_sched * sizeof(double), hipMemcpyHostToDevice, st));
    // every slot all ones, once per call: the rounds set back what they touch
    VCP_HIP(ctx, hipMemsetAsync(skey, 0xFF, slot_n * 12, st));
    VCP_HIP(ctx, hipMemsetAsync(d_lost, 0, (size_t)nst * sizeof(long long), st));
  }
  if (!grid) {  // the binary32 screening frame and copy serve the full scans only
    VCP_LAUNCH(ctx, k_model_frame, dim3(1), dim3(ITPB), 0, st, d_model, nm, d_st, nst);
    VCP_LAUNCH(ctx, k_model32, dim3(vcp_blocks(nm, ITPB)), dim3(ITPB), 0, st, d_model, nm, d_st, model32);
  }
  auto all_done = [&]() {
    for (int k = 0; k < nst; k++)
      if (!h_st[k].done) return false;
    return true;
  };
  int launched = 0;
  for (;;) {
    const int batch = mode == MODE_SUMS_ONLY ? 1 : std::min(all_rounds ? max_iter : ICP_BATCH, max_iter - launched);
    for (int b = 0; b < batch; b++) {
#define VCP_PASS(TBV, TL)                                                                                               \
  do {                                                                                                                  \
    if (ur) {                                                                                                           \
      if (phase == 0)                                                                                                   \
        VCP_LAUNCH(ctx, (k_icp_pass_uniq<TBV, TL, UniqDist>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,       \
                   (int)nm, d_data, nd, d_st, part, ng, ud);                                                            \
      else                                                                                                              \
        VCP_LAUNCH(ctx, (k_icp_pass_uniq<TBV, TL, UniqSum>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,        \
                   (int)nm, d_data, nd, d_st, part, ng, us);                                                            \
    } else if (tr) {                                                                                                    \
      if (phase == 0)                                                                                                   \
        VCP_LAUNCH(ctx, (k_icp_pass_trim<TBV, TL, TrimDist>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,       \
                   (int)nm, d_data, nd, d_st, part, ng, td);                                                            \
      else                                                                                                              \
        VCP_LAUNCH(ctx, (k_icp_pass_trim<TBV, TL, TrimSum>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,        \
                   (int)nm, d_data, nd, d_st, part, ng, ts);                                                            \
    } else if (sr)                                                                                                      \
      VCP_LAUNCH(ctx, (k_icp_pass_sim<TBV, TL>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32, (int)nm, d_data,   \
                 nd, d_st, part, d_nn, ng, sga);                                                                        \
    else if (gr)                                                                                                        \
      VCP_LAUNCH(ctx, (k_icp_pass_gated<TBV, TL>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32, (int)nm, d_data, \
                 nd, d_st, part, d_nn, ng, ga);                                                                         \
    else                                                                                                                \
      VCP_LAUNCH(ctx, (k_icp_pass<TBV, TL>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32, (int)nm, d_data, nd,   \
                 d_st, part, d_nn, ng);                                                                                 \
  } while (0)
#define VCP_PASS_SMALL(TBV)                                                                                             \
  do {                                                                                                                  \
    if (ur) {                                                                                                           \
      if (phase == 0)                                                                                                   \
        VCP_LAUNCH(ctx, (k_icp_pass_small_uniq<TBV, UniqDist>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,     \
                   (int)nm, d_data, nd, d_st, part, imask, tolk, ud);                                                   \
      else                                                                                                              \
        VCP_LAUNCH(ctx, (k_icp_pass_small_uniq<TBV, UniqSum>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,      \
                   (int)nm, d_data, nd, d_st, part, imask, tolk, us);                                                   \
    } else if (tr) {                                                                                                    \
      if (phase == 0)                                                                                                   \
        VCP_LAUNCH(ctx, (k_icp_pass_small_trim<TBV, TrimDist>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,     \
                   (int)nm, d_data, nd, d_st, part, imask, tolk, td);                                                   \
      else                                                                                                              \
        VCP_LAUNCH(ctx, (k_icp_pass_small_trim<TBV, TrimSum>), dim3(nb, nst), dim3(TBV), 0, st, d_model, model32,      \
                   (int)nm, d_data, nd, d_st, part, imask, tolk, ts);                                                   \
    } else if (sr)                                                                                                      \
      VCP_LAUNCH(ctx, k_icp_pass_small_sim<TBV>, dim3(nb, nst), dim3(TBV), 0, st, d_model, model32, (int)nm, d_data,   \
                 nd, d_st, part, d_nn, imask, tolk, sga);                                                               \
    else if (gr)                                                                                                        \
      VCP_LAUNCH(ctx, k_icp_pass_small_gated<TBV>, dim3(nb, nst), dim3(TBV), 0, st, d_model, model32, (int)nm, d_data, \
                 nd, d_st, part, d_nn, imask, tolk, ga);                                                                \
    else                                                                                                                \
      VCP_LAUNCH(ctx, k_icp_pass_small<TBV>, dim3(nb, nst), dim3(TBV), 0, st, d_model, model32, (int)nm, d_data, nd,   \
                 d_st, part, d_nn, imask, tolk);                                                                        \
  } while (0)
      // a trimmed round: the pass twice (distances, then sums) with the select between them; a unique-correspondence
      // round: likewise, with the tie pass between them
      for (int phase = 0; phase < (tr || ur ? 2 : 1); phase++) {
        if (small && grid) VCP_PASS(64, 2);
        else if (grid) VCP_PASS(ITPB, 2);
        else if (small && tiled) VCP_PASS(64, 1);
        else if (tiled) VCP_PASS(ITPB, 1);
        else if (small) VCP_PASS_SMALL(64);
        else VCP_PASS_SMALL(ITPB);
        if ((!tr && !ur) || phase == 1) break;
        if (ur) {
          VCP_LAUNCH(ctx, k_icpu_tie, dim3(vcp_blocks(nd, UNIQ_TIE_KEYS, UNIQ_TIE_BLOCKS), nst), dim3(ITPB), 0, st, d_st,
                     ud.a, nd);
        } else if (sel_wg) {
          VCP_LAUNCH(ctx, k_icpt_select_wg, dim3(nst), dim3(ITPB), 0, st, d_st, td.a, (int)nd);
        } else {
          const unsigned hb = vcp_blocks(nd, TRIM_HIST_KEYS, TRIM_HIST_BLOCKS);
          for (int d = 0; d < TRIM_DIGITS; d++)
            VCP_LAUNCH(ctx, k_icpt_hist, dim3(hb, nst), dim3(ITPB), 0, st, d_st, td.a, nd, d_ghist, d_slot, d);
          VCP_LAUNCH(ctx, k_icpt_select_fin, dim3(nst), dim3(ITPB), 0, st, d_st, td.a, d_ghist, d_slot);
        }
      }
#undef VCP_PASS
#undef VCP_PASS_SMALL
      if (ur) {  // sums only: one pass, nothing left to decide with the slots
        const bool reset = mode != MODE_SUMS_ONLY;
        if (reset && !reset_in_step)
          VCP_LAUNCH(ctx, k_icpu_reset, dim3(vcp_blocks(nd, UNIQ_TIE_KEYS, UNIQ_TIE_BLOCKS), nst), dim3(ITPB), 0, st, d_st,
                     ud.a, nd);
        VCP_LAUNCH(ctx, k_icp_step_unique, dim3(nst), dim3(ITPB), 0, st, part, nb, d_st, d_lost, ud.a,
                   (long long)(reset && reset_in_step ? nd : 0), gsa);
      } else if (tr) VCP_LAUNCH(ctx, k_icp_step_gated, dim3(nst), dim3(ITPB), 0, st, part, td.a.pkept, nb, d_st, gsa);
      else if (sr)
        VCP_LAUNCH(ctx, k_icp_step_sim, dim3(nst), dim3(ITPB), 0, st, part, ga.pkept, nb, d_st, d_side, gsa, ssa);
      else if (gr) VCP_LAUNCH(ctx, k_icp_step_gated, dim3(nst), dim3(ITPB), 0, st, part, ga.pkept, nb, d_st, gsa);
      else VCP_LAUNCH(ctx, k_icp_step, dim3(nst), dim3(ITPB), 0, st, part, nb, d_st, sa);
    }
    launched += batch;
    VCP_HIP(ctx, hipMemcpyAsync(h_st, d_st, (size_t)nst * sizeof(IcpState), hipMemcpyDeviceToHost, st));
    if (tr) VCP_HIP(ctx, hipMemcpyAsync(h_sel, td.a.sel, (size_t)nst * sizeof(TrimSel), hipMemcpyDeviceToHost, st));
    if (sr) VCP_HIP(ctx, hipMemcpyAsync(h_side, d_side, (size_t)nst * sizeof(SimSide), hipMemcpyDeviceToHost, st));
    if (ur) VCP_HIP(ctx, hipMemcpyAsync(h_lost, d_lost, (size_t)nst * sizeof(long long), hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    if (all_done() || launched >= max_iter || mode == MODE_SUMS_ONLY) break;
  }
  std::memcpy(out, h_st, (size_t)nst * sizeof(IcpState));
  if (tr) std::memcpy(tr->sel_out, h_sel, (size_t)nst * sizeof(TrimSel));
  if (sr) std::memcpy(sr->side_out, h_side, (size_t)nst * sizeof(SimSide));
  if (ur) std::memcpy(ur->lost_out, h_lost, (size_t)nst * sizeof(long long));
  for (int k = 0; k < nst; k++)
    if (out[k].failed) return vcp_fail(ctx, VCP_ERR_ARG, "Horn solve failed (non-finite sums)%s", nst > 1 ? " in a pose" : "");
  return VCP_OK;
}

// Inlier score of vcp_icp_multistart: grid (source points [x NNG lanes], poses).  Per pose h, M_h = [R_h | T_h] from the
// final state, then exactly k_match's arithmetic (match.hpp); a point counts when its nearest target is closer than
// max_dist.  One integer atomic per workgroup and pose: deterministic.
template <bool GRID>
__global__ __launch_bounds__(ITPB) void k_icpms_score(const double* __restrict__ src, int64_t ns,
                                                     const double* __restrict__ tgt, int nt,
                                                     const IcpState* __restrict__ st, double max_dist,
                                                     uint32_t* __restrict__ count, NNGrid ng) {
  constexpr int LPQ = GRID ? nng::NNG : 1;  // lanes per source point
  const int h = blockIdx.y;
  const int64_t j = ((int64_t)blockIdx.x * ITPB + threadIdx.x) / LPQ;
  const int sub = (int)(threadIdx.x & (LPQ - 1));
  double M[16];  // what vcp_icp_vtklike returns as M
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) M[4 * r + c] = st[h].R[3 * r + c];
    M[4 * r + 3] = st[h].T[r];
  }
  bool hit = false;
  if (j < ns) {  // uniform per NNG-lane group: the grid query's shuffles stay within live groups
    double m[3];
    mtc::transform(M, src[3 * j], src[3 * j + 1], src[3 * j + 2], m);
    int best;
    const double bd = mtc::nearest<GRID>(tgt, nt, ng, m, sub, best);
    hit = bd < max_dist && sub == 0;
  }
  __shared__ uint32_t wc[ITPB / 64];
  const unsigned long long b = __ballot(hit);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < ITPB / 64; w++) t += wc[w];
    if (t) atomicAdd(&count[h], t);
  }
}

}  // namespace

extern "C" {

int vcp_icp_dev(vcp_ctx* ctx, const double* d_model, int64_t nm, const double* d_data, int64_t nd, double tol,
                int max_iter, int stop_rule, double R[9], double T[3], double* sse_o, double* rmse_o,
                int32_t* iters_o) {
  if (!ctx) return VCP_ERR_ARG;
  if (nm <= 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "empty model (model[0], BaseClass/ICP.cs:233)");
  if (nd < 0 || max_iter < 1 || !R || !T) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (nm >= 0x7FFFFFFFLL / 3 || nd >= ((int64_t)1 << 40)) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "too many points");
  if (stop_rule != VCP_STOP_SSE_DELTA && stop_rule != VCP_STOP_RMSE) return vcp_fail(ctx, VCP_ERR_ARG, "stop_rule");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (nd == 0) {  // the C# divides by zero: NaN sums, |NaN - 0| >= e is false, one round, R and T untouched
    if (sse_o) *sse_o = 0.0;
    if (rmse_o) *rmse_o = 0.0;
    if (iters_o) *iters_o = 1;
    ctx->last_timing.clear();
    return VCP_OK;
  }
  vcp_phase(ctx, "icp_rounds");
  IcpState init, fin;
  identity(init);  // round 1 matches the raw data (P = copy of data, :22); 1*x + 0*y + 0*z is exact
  VCP_TRY(icp_run(ctx, d_model, nm, d_data, nd, &init, 1, tol, stop_rule, max_iter, MODE_REFERENCE, &fin, nullptr, false,
                  nullptr));
  VCP_TRY(vcp_phase_finish(ctx));
  // R, T are written once some round has asked to continue (:149-162); if round 1 already stops they stay
  // whatever the caller passed in
  const bool wrote = fin.round > 1 || (stop_rule == VCP_STOP_RMSE ? std::sqrt(fin.d / (double)nd) >= tol
                                                                    : std::fabs(fin.d) >= tol);
  if (wrote) {
    std::memcpy(R, fin.R, sizeof(fin.R));
    std::memcpy(T, fin.T, sizeof(fin.T));
  }
  if (sse_o) *sse_o = fin.d;
  if (rmse_o) *rmse_o = std::sqrt(fin.d / (double)nd);
  if (iters_o) *iters_o = fin.round;
  return VCP_OK;
}

int vcp_icp(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, double tol, int max_iter,
            int stop_rule, double R[9], double T[3], double* sse, double* rmse, int32_t* iters) {
  if (!ctx) return VCP_ERR_ARG;
  if (nm <= 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "empty model (model[0], BaseClass/ICP.cs:233)");
  if (nd < 0 || !model || (nd > 0 && !data)) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  VCP_TRY(vcp_bind(ctx));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)nm * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, (size_t)(nd > 0 ? nd : 1) * 24));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, model, (size_t)nm * 24, hipMemcpyHostToDevice, ctx->stream));
  if (nd > 0) VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, data, (size_t)nd * 24, hipMemcpyHostToDevice, ctx->stream));
  return vcp_icp_dev(ctx, ctx->b_in0.as<double>(), nm, ctx->b_in2.as<double>(), nd, tol, max_iter, stop_rule, R, T,
                     sse, rmse, iters);
}

// "VTK-like" configuration of the same loop: what MainForm.ICP() asks of
// vtkIterativeClosestPointTransform (FrmMain.cs:851-862: RigidBody, 100 iterations, StartByMatchingCentroidsOn,
// no mean-distance check), following the VTK 5.0 header (vtkIterativeClosestPointTransform.h:49-180): landmarks =
// every step-th source point (step = ns / max_landmarks when ns > max_landmarks), optional initial translation
// target centroid - source centroid, max_iter rounds, accumulated 4x4 matrix.  VTK's sources are not in the
// reference tree: behaviour per the header only, PARITY UNPINNED against VTK itself.
int vcp_icp_vtklike(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int max_iter,
                    int max_landmarks, int start_by_matching_centroids, double M[16], double* mean_dist,
                    int32_t* iters_o) {
  if (!ctx) return VCP_ERR_ARG;
  if (ns <= 0 || nt <= 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "empty source or target");
  if (max_iter < 1 || max_landmarks < 1 || !source || !target || !M) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (nt >= 0x7FFFFFFFLL / 3) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "target too large");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  int64_t step = 1;
  if (ns > max_landmarks) step = ns / max_landmarks;
  const int64_t nb = ns / step;
  std::vector<double> a((size_t)3 * nb);
  for (int64_t i = 0, j = 0; i < nb; i++, j += step)
    for (int c = 0; c < 3; c++) a[3 * i + c] = source[3 * j + c];
  IcpState init, fin;
  identity(init);
  if (start_by_matching_centroids) {  // sequential binary64 means over ALL points of both sets
    double cs[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
    for (int64_t i = 0; i < ns; i++)
      for (int c = 0; c < 3; c++) cs[c] += source[3 * i + c];
    for (int64_t i = 0; i < nt; i++)
      for (int c = 0; c < 3; c++) ct[c] += target[3 * i + c];
    for (int c = 0; c < 3; c++) init.T[c] = ct[c] / (double)nt - cs[c] / (double)ns;
  }
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)nt * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, (size_t)nb * 24));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, target, (size_t)nt * 24, hipMemcpyHostToDevice, ctx->stream));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, a.data(), (size_t)nb * 24, hipMemcpyHostToDevice, ctx->stream));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `a` is a local buffer
  VCP_TRY(icp_run(ctx, ctx->b_in0.as<double>(), nt, ctx->b_in2.as<double>(), nb, &init, 1, 0.0, VCP_STOP_SSE_DELTA,
                  max_iter, MODE_VTK, &fin, nullptr, false, nullptr));
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * r + c] = fin.R[3 * r + c];
    M[4 * r + 3] = fin.T[r];
  }
  M[12] = M[13] = M[14] = 0;
  M[15] = 1;
  if (mean_dist) *mean_dist = std::sqrt(fin.d / (double)nb);
  if (iters_o) *iters_o = fin.round;
  return VCP_OK;
}

// Multi-start form of vcp_icp_vtklike (vcp.h): the same landmarks, rounds and arithmetic per pose, from H starts at
// once; the target's grid (or screening frame) is built once and serves every pose and the score.
// gr (NULL: vcp_icp_multistart): the gated form, vcp_icp_gated -- its schedule is checked here, next to the other
// arguments, and kept / starved (each may be NULL) receive the states' counters.
// tr (never with gr): the trimmed form, vcp_icp_trimmed -- likewise, and trim_dist (may be NULL) receives the root of
// the last round's thr.
// sr (only with gr): the similarity form, vcp_icp_sim -- its bounds are checked here, and ratio / unscaled (each may be
// NULL) receive the side records' c and count.
// ur (never with gr or tr): the unique-correspondence form, vcp_icp_unique -- its schedule is checked as gr's is, and
// lost (may be NULL) receives the last round's count of pairs that were not their target's winner.
static bool sim_range_ok(double ratio_min, double ratio_max) {
  return ratio_min > 0.0 && ratio_max >= ratio_min && ratio_max <= 1.7976931348623157e308;  // false for NaN
}
static int icp_multistart_run(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                              int32_t n_poses, const double* init_R, const double* init_T, int max_iter,
                              int max_landmarks, double inlier_dist, double M_best[16], int32_t* best, double* M_all,
                              double* mean_dist, int32_t* inliers, const GateRun* gr, int64_t* kept, int32_t* starved,
                              const TrimRun* tr = nullptr, double* trim_dist = nullptr, const SimRun* sr = nullptr,
                              double* ratio = nullptr, int32_t* unscaled = nullptr, const UniqRun* ur = nullptr,
                              int64_t* lost = nullptr) {
  if (!ctx) return VCP_ERR_ARG;
  if (ns <= 0 || nt <= 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "empty source or target");
  if (max_iter < 1 || max_landmarks < 1 || !source || !target || !M_best || !best)
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (nt >= 0x7FFFFFFFLL / 3) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "target too large");
  if (n_poses < 1) return vcp_fail(ctx, VCP_ERR_ARG, "n_poses < 1");
  if (n_poses > ICPMS_MAX_POSES) return vcp_fail(ctx, VCP_ERR_UNSUPPORTED, "n_poses > %d", ICPMS_MAX_POSES);
  if (!(inlier_dist > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "inlier_dist must be > 0 (+inf allowed)");
  for (int64_t k = 0; k < (int64_t)n_poses * 9 && init_R; k++)
    if (!std::isfinite(init_R[k])) return vcp_fail(ctx, VCP_ERR_ARG, "non-finite init_R");
  for (int64_t k = 0; k < (int64_t)n_poses * 3 && init_T; k++)
    if (!std::isfinite(init_T[k])) return vcp_fail(ctx, VCP_ERR_ARG, "non-finite init_T");
  if (gr) {
    if (gr->n_gates < 1 || !gr->gates) return vcp_fail(ctx, VCP_ERR_ARG, "n_gates < 1");
    if (gr->min_pairs < 1) return vcp_fail(ctx, VCP_ERR_ARG, "min_pairs < 1");
    for (int k = 0; k < gr->n_gates; k++)
      if (!(gr->gates[k] > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "gates must be > 0 (+inf allowed)");
  }
  if (ur) {
    if (ur->n_gates < 1 || !ur->gates) return vcp_fail(ctx, VCP_ERR_ARG, "n_gates < 1");
    if (ur->min_pairs < 1) return vcp_fail(ctx, VCP_ERR_ARG, "min_pairs < 1");
    for (int k = 0; k < ur->n_gates; k++)
      if (!(ur->gates[k] > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "gates must be > 0 (+inf allowed)");
  }
  if (sr) {
    if (!sim_range_ok(sr->ratio_min, sr->ratio_max))
      return vcp_fail(ctx, VCP_ERR_ARG, "need 0 < ratio_min <= ratio_max < inf");
    if (!(sr->ratio_min <= 1.0 && 1.0 <= sr->ratio_max))
      return vcp_fail(ctx, VCP_ERR_ARG, "need ratio_min <= 1 <= ratio_max");
  }
  if (tr) {
    if (tr->n_share < 1 || !tr->share) return vcp_fail(ctx, VCP_ERR_ARG, "n_keep < 1");
    if (tr->min_pairs < 1) return vcp_fail(ctx, VCP_ERR_ARG, "min_pairs < 1");
    for (int k = 0; k < tr->n_share; k++)
      if (!(tr->share[k] > 0.0 && tr->share[k] <= 1.0)) return vcp_fail(ctx, VCP_ERR_ARG, "keep shares must be in (0, 1]");
  }
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  vcp_phase(ctx, ur ? "icpu_rounds" : tr ? "icpt_rounds" : sr ? "icps_rounds" : gr ? "icpg_rounds" : "icpms_rounds");
  int64_t step = 1;
  if (ns > max_landmarks) step = ns / max_landmarks;
  const int64_t nb = ns / step;
  std::vector<double> a((size_t)3 * nb);
  for (int64_t i = 0, j = 0; i < nb; i++, j += step)
    for (int c = 0; c < 3; c++) a[3 * i + c] = source[3 * j + c];
  // source and target means exactly as vcp_icp_vtklike's centroid start computes them
  double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
  if (!init_T) {
    for (int64_t i = 0; i < ns; i++)
      for (int c = 0; c < 3; c++) ms[c] += source[3 * i + c];
    for (int64_t i = 0; i < nt; i++)
      for (int c = 0; c < 3; c++) mt[c] += target[3 * i + c];
    for (int c = 0; c < 3; c++) {
      ms[c] = ms[c] / (double)ns;
      mt[c] = mt[c] / (double)nt;
    }
  }
  std::vector<IcpState> init((size_t)n_poses), fin((size_t)n_poses);
  std::vector<TrimSel> sel(tr ? (size_t)n_poses : 0);
  TrimRun trun{};
  if (tr) {
    trun = *tr;
    trun.sel_out = sel.data();
  }
  std::vector<SimSide> side(sr ? (size_t)n_poses : 0);
  SimRun srun{};
  if (sr) {
    srun = *sr;
    srun.side_out = side.data();
  }
  std::vector<long long> nlost(ur ? (size_t)n_poses : 0);
  UniqRun urun{};
  if (ur) {
    urun = *ur;
    urun.lost_out = nlost.data();
  }
  for (int h = 0; h < n_poses; h++) {
    IcpState& s = init[h];
    identity(s);
    if (init_R) {
      std::memcpy(s.R, init_R + 9 * (size_t)h, sizeof(s.R));
    } else {  // Rz(theta_h); 0 - s keeps h = 0 exactly the identity (no -0)
      const double th = (double)h * (2.0 * M_PI / (double)n_poses), c = std::cos(th), sn = std::sin(th);
      const double R0[9] = {c, 0.0 - sn, 0.0, sn, c, 0.0, 0.0, 0.0, 1.0};
      std::memcpy(s.R, R0, sizeof(s.R));
    }
    if (init_T) {
      std::memcpy(s.T, init_T + 3 * (size_t)h, sizeof(s.T));
    } else {  // T0 = mt - R0 ms, R0 ms row by row, left to right
      for (int r = 0; r < 3; r++) s.T[r] = mt[r] - (s.R[3 * r] * ms[0] + s.R[3 * r + 1] * ms[1] + s.R[3 * r + 2] * ms[2]);
    }
  }
  hipStream_t st = ctx->stream;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)nt * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, (size_t)nb * 24));
  if (step > 1) VCP_TRY(vcp_ensure(ctx, ctx->b_in3, (size_t)ns * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, (size_t)n_poses * 4));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, target, (size_t)nt * 24, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, a.data(), (size_t)nb * 24, hipMemcpyHostToDevice, st));
  if (step > 1) VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in3.p, source, (size_t)ns * 24, hipMemcpyHostToDevice, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));  // `a` is a local buffer
  NNGrid ng{};
  VCP_TRY(icp_run(ctx, ctx->b_in0.as<double>(), nt, ctx->b_in2.as<double>(), nb, init.data(), n_poses, 0.0,
                  VCP_STOP_SSE_DELTA, max_iter, MODE_VTK, fin.data(), nullptr, true, &ng, gr, tr ? &trun : nullptr,
                  sr ? &srun : nullptr, ur ? &urun : nullptr));
  // score every pose over ALL source points with vcp_match's arithmetic, on the grid the rounds used (vcp_match bins
  // a target of more than 512 points too, and falls back to the full scan on the same condition)
  vcp_phase(ctx, ur ? "icpu_score" : tr ? "icpt_score" : sr ? "icps_score" : gr ? "icpg_score" : "icpms_score");
  const double* d_src = step > 1 ? ctx->b_in3.as<double>() : ctx->b_in2.as<double>();  // step 1: the landmarks are all
  const IcpState* d_st = icp_states(ctx);
  uint32_t* d_cnt = ctx->b_out0.as<uint32_t>();
  VCP_HIP(ctx, hipMemsetAsync(d_cnt, 0, (size_t)n_poses * 4, st));
  if (ng.rec)
    VCP_LAUNCH(ctx, k_icpms_score<true>, dim3(vcp_blocks(ns * nng::NNG, ITPB), n_poses), dim3(ITPB), 0, st, d_src, ns,
               ctx->b_in0.as<double>(), (int)nt, d_st, inlier_dist, d_cnt, ng);
  else
    VCP_LAUNCH(ctx, k_icpms_score<false>, dim3(vcp_blocks(ns, ITPB), n_poses), dim3(ITPB), 0, st, d_src, ns,
               ctx->b_in0.as<double>(), (int)nt, d_st, inlier_dist, d_cnt, ng);
  uint32_t* h_cnt = reinterpret_cast<uint32_t*>(vcp_stage(ctx, (size_t)n_poses * 4));
  if (!h_cnt) return vcp_fail(ctx, VCP_ERR_NOMEM, "pinned staging of the scores");
  VCP_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, (size_t)n_poses * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  VCP_TRY(vcp_phase_finish(ctx));
  // RMS distance of the pairs the last round summed: all nb landmarks, or the kept ones of a gated run (none: +inf)
  auto mean_of = [&](const IcpState& f) {
    if (!gr && !tr && !ur) return std::sqrt(f.d / (double)nb);
    return f.kept > 0 ? std::sqrt(f.d / (double)f.kept) : (double)INFINITY;
  };
  // most inliers, then the smaller mean distance, then the lower index
  int b = 0;
  for (int h = 0; h < n_poses; h++) {
    const double md = mean_of(fin[h]), mb = mean_of(fin[b]);
    if (h_cnt[h] > h_cnt[b] || (h_cnt[h] == h_cnt[b] && md < mb)) b = h;
    if (M_all) {
      double* M = M_all + 16 * (size_t)h;
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) M[4 * r + c] = fin[h].R[3 * r + c];
        M[4 * r + 3] = fin[h].T[r];
      }
      M[12] = M[13] = M[14] = 0;
      M[15] = 1;
    }
    if (mean_dist) mean_dist[h] = md;
    if (inliers) inliers[h] = (int32_t)h_cnt[h];
    if (kept) kept[h] = (int64_t)fin[h].kept;
    if (starved) starved[h] = fin[h].starved;
    if (sr && ratio) ratio[h] = side[h].c;
    if (sr && unscaled) unscaled[h] = side[h].unscaled;
    if (ur && lost) lost[h] = (int64_t)nlost[h];
    if (tr && trim_dist) {
      double thr;
      std::memcpy(&thr, &sel[h].key, sizeof(thr));
      trim_dist[h] = std::sqrt(thr);
    }
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M_best[4 * r + c] = fin[b].R[3 * r + c];
    M_best[4 * r + 3] = fin[b].T[r];
  }
  M_best[12] = M_best[13] = M_best[14] = 0;
  M_best[15] = 1;
  *best = b;
  return VCP_OK;
}

int vcp_icp_multistart(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                       int32_t n_poses, const double* init_R, const double* init_T, int max_iter, int max_landmarks,
                       double inlier_dist, double M_best[16], int32_t* best, double* M_all, double* mean_dist,
                       int32_t* inliers) {
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, nullptr, nullptr, nullptr);
}

// vcp_icp_multistart with a per-round gate on the correspondence distance (vcp.h)
int vcp_icp_gated(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                  const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                  int32_t n_gates, int32_t min_pairs, double inlier_dist, double M_best[16], int32_t* best,
                  double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved) {
  const GateRun gr{gates, n_gates, min_pairs, nullptr};
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, &gr, kept, starved);
}

// vcp_icp_multistart with a per-round keep share: every round fits on the closest pairs alone (vcp.h)
int vcp_icp_trimmed(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                    const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* keep,
                    int32_t n_keep, int32_t min_pairs, double inlier_dist, double M_best[16], int32_t* best,
                    double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved,
                    double* trim_dist) {
  const TrimRun tr{keep, n_keep, 0, min_pairs, nullptr, nullptr};
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, nullptr, kept, starved, &tr, trim_dist);
}

// vcp_icp_gated whose rounds fit one isotropic scale beside the rotation and the translation (vcp.h)
int vcp_icp_sim(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                int32_t n_gates, int32_t min_pairs, double ratio_min, double ratio_max, double inlier_dist,
                double M_best[16], int32_t* best, double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept,
                int32_t* starved, double* ratio, int32_t* unscaled) {
  const GateRun gr{gates, n_gates, min_pairs, nullptr};
  const SimRun sr{ratio_min, ratio_max, nullptr};
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, &gr, kept, starved, nullptr, nullptr, &sr, ratio,
                            unscaled);
}

// vcp_icp_gated where, of the landmarks that share a nearest target, only the closest enters a round's sums (vcp.h)
int vcp_icp_unique(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                   const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                   int32_t n_gates, int32_t min_pairs, double inlier_dist, double M_best[16], int32_t* best,
                   double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved, int64_t* lost) {
  const UniqRun ur{gates, n_gates, min_pairs, nullptr, nullptr};
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, nullptr, kept, starved, nullptr, nullptr, nullptr,
                            nullptr, nullptr, &ur, lost);
}

// Host-side run of the Horn step the device executes per round (same source: horn() is __host__ __device__).
int vcp_selftest_horn(const double sums[16], int64_t nd, double V[16], int use_v, double R1[9], double T1[3]) {
  if (!sums || !R1 || !T1 || nd <= 0 || (use_v && !V)) return VCP_ERR_ARG;
  return horn(sums, (long long)nd, R1, T1, use_v ? V : nullptr) ? 1 : 0;
}

// Host-side run of the similarity step (horn_sim is __host__ __device__ too).  Returns 0, 1 or 2 as horn_sim does.
int vcp_selftest_horn_sim(const double sums[18], int64_t n, double V[16], int use_v, double c, double ratio_min,
                          double ratio_max, double R1s[9], double T1[3], double* k_used, double* c_new) {
  if (!sums || !R1s || !T1 || !k_used || !c_new || n <= 0 || (use_v && !V)) return VCP_ERR_ARG;
  if (!(c > 0.0) || !sim_range_ok(ratio_min, ratio_max)) return VCP_ERR_ARG;
  return horn_sim(sums, (long long)n, c, ratio_min, ratio_max, R1s, T1, use_v ? V : nullptr, k_used, c_new);
}

// gate (NULL: vcp_icp_sums): one gated pass, vcp_icp_sums_gated; kept and keep receive its verdicts
// m (never with gate): one trimmed round's passes, vcp_icp_sums_trimmed; thr_dd and keep receive its verdicts
// lost (only with gate): one unique-correspondence round's passes, vcp_icp_sums_unique; kept, lost and keep receive
// its verdicts
static int icp_sums_run(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                        const double T[3], double sums[16], int32_t* nn, const double* gate, int64_t* kept,
                        uint8_t* keep, const int64_t* m = nullptr, double* thr_dd = nullptr, bool sim = false,
                        int64_t* lost = nullptr) {
  if (!ctx) return VCP_ERR_ARG;
  if (nm <= 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "empty model");
  if (nd <= 0 || !model || !data || !sums) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (nm >= 0x7FFFFFFFLL / 3) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "model too large");
  if (gate && !(*gate > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "gate must be > 0 (+inf allowed)");
  if (gate && !kept) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (m && !thr_dd) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (m && (*m < 1 || *m > nd)) return vcp_fail(ctx, VCP_ERR_ARG, "m must be in [1, nd]");
  if ((m || lost) && nd > 0xFFFFFFFFLL)
    return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "the key holds the landmark in 32 bits");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)nm * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, (size_t)nd * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, (size_t)nd * 4));
  if (keep) VCP_TRY(vcp_ensure(ctx, ctx->b_out1, (size_t)nd));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, model, (size_t)nm * 24, hipMemcpyHostToDevice, ctx->stream));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, data, (size_t)nd * 24, hipMemcpyHostToDevice, ctx->stream));
  IcpState init, fin;
  identity(init);
  if (R) std::memcpy(init.R, R, sizeof(init.R));
  if (T) std::memcpy(init.T, T, sizeof(init.T));
  const GateRun gr{gate, 1, 1, keep ? ctx->b_out1.as<uint8_t>() : nullptr};
  TrimSel sel{};
  const TrimRun tr{nullptr, 0, m ? (long long)*m : 0, 1, keep ? ctx->b_out1.as<uint8_t>() : nullptr, &sel};
  SimSide side{};
  const SimRun sr{1.0, 1.0, &side};  // sim (only with gate): the 18-wide pass, sums [18]
  long long nlost = 0;
  const UniqRun ur{gate, 1, 1, keep ? ctx->b_out1.as<uint8_t>() : nullptr, &nlost};
  const bool stored_nn = m || lost;  // the rounds that keep the index found in their own workspace
  VCP_TRY(icp_run(ctx, ctx->b_in0.as<double>(), nm, ctx->b_in2.as<double>(), nd, &init, 1, 0.0, VCP_STOP_SSE_DELTA, 1,
                  MODE_SUMS_ONLY, &fin, nn && !stored_nn ? ctx->b_out0.as<int32_t>() : nullptr, false, nullptr,
                  gate && !lost ? &gr : nullptr, m ? &tr : nullptr, sim ? &sr : nullptr, lost ? &ur : nullptr));
  std::memcpy(sums, fin.sums, sizeof(fin.sums));
  if (sim) {
    sums[16] = side.s16;
    sums[17] = side.s17;
  }
  if (gate) *kept = (int64_t)fin.kept;
  if (lost) *lost = (int64_t)nlost;
  if (m) std::memcpy(thr_dd, &sel.key, sizeof(double));
  if (stored_nn) {
    if (nn) VCP_HIP(ctx, hipMemcpyAsync(nn, icpt_nn(ctx, 1, nd), (size_t)nd * 4, hipMemcpyDeviceToHost, ctx->stream));
  } else if (nn) {
    VCP_HIP(ctx, hipMemcpyAsync(nn, ctx->b_out0.p, (size_t)nd * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (keep) VCP_HIP(ctx, hipMemcpyAsync(keep, ctx->b_out1.p, (size_t)nd, hipMemcpyDeviceToHost, ctx->stream));
  if (nn || keep) VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_icp_sums(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                 const double T[3], double sums[16], int32_t* nn) {
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, nullptr, nullptr, nullptr);
}

int vcp_icp_sums_gated(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                       const double T[3], double gate, double sums[16], int64_t* kept, int32_t* nn, uint8_t* keep) {
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, &gate, kept, keep);
}

int vcp_icp_sums_sim(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                     const double T[3], double gate, double sums[18], int64_t* kept, int32_t* nn, uint8_t* keep) {
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, &gate, kept, keep, nullptr, nullptr, true);
}

int vcp_icp_sums_unique(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                        const double T[3], double gate, double sums[16], int64_t* kept, int32_t* nn, uint8_t* keep,
                        int64_t* lost) {
  if (ctx && !lost) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, &gate, kept, keep, nullptr, nullptr, false, lost);
}

int vcp_icp_sums_trimmed(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                         const double R[9], const double T[3], int64_t m, double sums[16], double* thr_dd, int32_t* nn,
                         uint8_t* keep) {
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, nullptr, nullptr, keep, &m, thr_dd);
}

}  // extern "C"
