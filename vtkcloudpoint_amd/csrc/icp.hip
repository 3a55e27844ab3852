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
// Forms (vcp.h: gated, similarity, trimmed, unique-correspondence, anisotropic ICP): a form is a POLICY type, the last
// argument of the two pass kernels k_icp_pass<TB, NNMODE, G> and k_icp_pass_small<TB, G>.  The policy says at compile
// time whether the pass searches, sums, stores keys, counts kept pairs; the bodies share one per-pair function
// (icp_pair: the keep rule and the 16 or 18 accumulations, written once, over p or -- the anisotropic form -- over the
// raw landmark) and one epilogue.  The plain policy NoGate is empty.  The forms
// that count their kept pairs share one step, k_icp_step_kept<F>, whose FORM type F holds what a form adds to it.  On
// the host one IcpVariant names the form of a run, icp_layout() places everything a run keeps in the workspace, and
// PassLaunch launches a pass on the path the run has chosen.  The Horn solve itself lives in horn.hpp.
//
// Nearest neighbour: the model index is wave-uniform, so model points come through the scalar cache, four per
// trip.  Distances are first screened in binary32 (three FMAs per pair) with a rigorous rounding bound; only model points whose
// binary32 distance is within that bound of the smallest are re-evaluated in binary64, in index order with the
// C#'s strict `<` -- the chosen index is bit-identical to a full binary64 scan.
// Algorithmic bytes: 24 B per data point per round; at 1M x 100 the pass is VALU bound, not HBM bound.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "horn.hpp"
#include "match.hpp"
#include "nngrid.hpp"
#include "radix_pick.hpp"
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

// ---- the policies of a pass --------------------------------------------------------------------------------------
// Both pass kernels are compiled once per POLICY, the type of their last argument: it holds what that form of the pass
// reads beside the state, and says at compile time what the pass does.
//   SEARCH  it runs the NN search (false: it reads the index a distance pass stored)
//   SUMS    it accumulates NS columns and folds them into the workgroup's partial row
//   STORE   it stores K(dd) and the index found per landmark: store(view, i, order, K)
//   COUNT   it decides per pair whether the pair enters the sums, keeps(view, i, order, dd, code, nlost), writes the
//           verdict to keep[] (if not NULL) and the workgroup's count of kept pairs to pkept
//   LOST    it also counts the pairs that are not their target's winner, into plost
//   NS      columns of a row
//   RAW     (COUNT policies) the d-side columns (0..2, the rows of 6..14, 16, 17) sum the landmark d as read, not p
//   view(st, nd)  what the pass needs of its pose (blockIdx.y), read once before the loop
// A dropped pair adds +0.0 to each row at its own place in the tree, which therefore stays the ungated one.
struct PoseView {
  double gate;              // this round's gate
  unsigned long long* key;  // [L]: K(dd) per landmark of the pose
  int32_t* nn;              // [L]: the index found
  unsigned long long thrk;  // trimmed: the selected key
  uint32_t thri;            // and its landmark
  unsigned long long* skey;  // unique: [nt] the pose's slots
  const uint32_t* sidx;
};
// round r (1-based) uses sched[min(r, n) - 1]; the state's round counter says which
__device__ __forceinline__ double sched_now(const double* sched, int n, const IcpState* st) {
  return sched[min(st->round + 1, n) - 1];
}
__device__ __forceinline__ PoseView stored_view(unsigned long long* key, int32_t* nn, int64_t nd) {
  PoseView v{};
  v.key = key + (size_t)blockIdx.y * (size_t)nd;
  v.nn = nn + (size_t)blockIdx.y * (size_t)nd;
  return v;
}

// The plain pass: every pair enters the sums, unconditionally.  Empty: the kernels' other arguments lie where they did.
struct NoGate {
  static constexpr bool SEARCH = true, SUMS = true, STORE = false, COUNT = false, LOST = false;
  static constexpr int NS = 16;
  __device__ __forceinline__ PoseView view(const IcpState*, int64_t) const { return PoseView{}; }
};
// The gated pass (vcp.h, vcp_icp_gated): the schedule on the device, one kept count per workgroup next to its partial
// row, and optionally the per-point verdict.  A pair whose distance sqrt(dd) is >= the round's gate is dropped; dd is
// the SSE term.  A NaN dd compares false: kept.
struct GateArgs {
  static constexpr bool SEARCH = true, SUMS = true, STORE = false, COUNT = true, LOST = false, RAW = false;
  static constexpr int NS = 16;
  const double* gates;
  int n_gates;
  uint32_t* pkept;  // [poses][workgroups]
  uint8_t* keep;    // [nd] or NULL
  __device__ __forceinline__ PoseView view(const IcpState* st, int64_t) const {
    PoseView v{};
    v.gate = sched_now(gates, n_gates, st);
    return v;
  }
  __device__ __forceinline__ bool keeps(const PoseView& v, int64_t, int, double dd, uint8_t& code, uint32_t&) const {
    const bool kp = !(sqrt(dd) >= v.gate);
    code = kp ? 1 : 0;
    return kp;
  }
};
// Similarity ICP (vcp.h, "similarity ICP"): the gated pass with two more columns, sum |p|^2 at 16 and sum |y|^2 at 17,
// through the same tree.  A type of its own: the kernels of GateArgs stay the 16-wide ones they were.
struct SimGate : GateArgs {
  static constexpr int NS = 18;
};
// Anisotropic ICP (vcp.h, "anisotropic ICP"): the gated pass whose d-side columns sum the RAW landmark d where the
// others sum p = A d + T (the pair, the distance and the gate stay p's), with sum d0^2 at 16 and sum d1^2 at 17.  Its
// step sets the pose from those sums; it composes nothing.
struct AnisoGate : GateArgs {
  static constexpr int NS = 18;
  static constexpr bool RAW = true;
};

// Trimmed ICP (vcp.h, "trimmed ICP"): a round keeps the m landmarks with the smallest 96-bit keys [K(dd) | index].
// Three steps per round and pose: a pass that runs the NN search and stores K(dd) and the index found (TrimDist), a
// radix select of the rank-m key (k_icpt_select_wg, or k_icpt_hist x 12 + k_icpt_select_fin), and the sums pass
// (TrimSum), which reads both back and keeps "key <= the selected one" where the gated pass tests the distance.
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
struct TrimDist : TrimArgs {
  static constexpr bool SEARCH = true, SUMS = false, STORE = true, COUNT = false, LOST = false;
  static constexpr int NS = 16;
  __device__ __forceinline__ PoseView view(const IcpState*, int64_t nd) const { return stored_view(key, nn, nd); }
  __device__ __forceinline__ void store(const PoseView& v, int64_t i, int order, unsigned long long k) const {
    v.key[i] = k;
    v.nn[i] = order;
  }
};
struct TrimSum : TrimArgs {
  static constexpr bool SEARCH = false, SUMS = true, STORE = false, COUNT = true, LOST = false, RAW = false;
  static constexpr int NS = 16;
  __device__ __forceinline__ PoseView view(const IcpState*, int64_t nd) const {
    PoseView v = stored_view(key, nn, nd);
    v.thrk = sel[blockIdx.y].key;
    v.thri = sel[blockIdx.y].idx;
    return v;
  }
  __device__ __forceinline__ bool keeps(const PoseView& v, int64_t i, int, double, uint8_t& code, uint32_t&) const {
    const unsigned long long k = v.key[i];
    const bool kp = k < v.thrk || (k == v.thrk && (uint32_t)i <= v.thri);
    code = kp ? 1 : 0;
    return kp;
  }
};

// Unique-correspondence ICP (vcp.h, "unique-correspondence ICP"): of the landmarks that share a nearest target, only the
// one with the smallest 96-bit key [K(dd) | index] -- the target's WINNER -- may enter the sums; the gate then decides
// on the winner as it does in the gated pass.  Three steps per round and pose: a pass that runs the NN search, stores
// K(dd) and the index found and takes the 64-bit minimum of K(dd) in the slot of (pose, target) (UniqDist); the tie
// pass k_icpu_tie, the 32-bit minimum of the landmark among those whose K equals the slot's; and the sums pass
// (UniqSum), which keeps "my key and my index are the slot's, and the gate keeps me".  A slot is 12 bytes, two
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
struct UniqDist : UniqArgs {
  static constexpr bool SEARCH = true, SUMS = false, STORE = true, COUNT = false, LOST = false;
  static constexpr int NS = 16;
  __device__ __forceinline__ PoseView view(const IcpState*, int64_t nd) const {
    PoseView v = stored_view(key, nn, nd);
    v.skey = skey + (size_t)blockIdx.y * (size_t)nt;
    return v;
  }
  __device__ __forceinline__ void store(const PoseView& v, int64_t i, int order, unsigned long long k) const {
    v.key[i] = k;
    v.nn[i] = order;
    atomicMin(v.skey + (size_t)order, k);
  }
};
struct UniqSum : UniqArgs {
  static constexpr bool SEARCH = false, SUMS = true, STORE = false, COUNT = true, LOST = true, RAW = false;
  static constexpr int NS = 16;
  __device__ __forceinline__ PoseView view(const IcpState* st, int64_t nd) const {
    PoseView v = stored_view(key, nn, nd);
    v.gate = sched_now(gates, n_gates, st);
    v.skey = skey + (size_t)blockIdx.y * (size_t)nt;
    v.sidx = sidx + (size_t)blockIdx.y * (size_t)nt;
    return v;
  }
  __device__ __forceinline__ bool keeps(const PoseView& v, int64_t i, int order, double dd, uint8_t& code, uint32_t& nlost) const {
    const bool win = v.key[i] == v.skey[order] && (uint32_t)i == v.sidx[order];
    const bool kp = win && !(sqrt(dd) >= v.gate);
    nlost += win ? 0u : 1u;
    code = win ? (kp ? 1 : 0) : 2;
    return kp;
  }
};

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
// The keep count of the round a trimmed kernel runs now: min(L, ceil(f * L)), one multiplication; f in (0, 1] (checked
// on the host), so the count lies in [1, L].
__device__ __forceinline__ long long trim_m(const TrimArgs& a, const IcpState* st, long long L) {
  if (a.m_fixed > 0) return a.m_fixed;
  const double f = sched_now(a.share, a.n_share, st);
  const long long m = (long long)ceil(f * (double)L);
  return m < L ? m : L;
}
// A workgroup's count written next to its partial row (wave shuffle, then the waves in order: integers, exact in any
// order).
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

// ---- what the two pass bodies share: everything but the search --------------------------------------------------
// TransPoint: r = R*p accumulated k ascending from 0 (Matrix.StupidMultiply), then + T
__device__ __forceinline__ void trans_point(const double (&R)[9], const double (&T)[3], double d0, double d1, double d2,
                                            double (&p)[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double acc = 0.0;
    acc += R[3 * r] * d0;
    acc += R[3 * r + 1] * d1;
    acc += R[3 * r + 2] * d2;
    p[r] = acc + T[r];
  }
}

// More than one candidate within the bound `lim` of the screening (or non-finite values): exact binary64 among the
// candidates, in index order, strict `<` -- FindClosestPointSet's rule (the C# seeds with model[0] and replaces on `<`,
// so the lowest index among the exact minima wins; every exact minimum is a candidate by the bound)
__device__ __forceinline__ int icp_exact_scan(const double* model, const float4* model32, int nm, float q0, float q1,
                                              float q2, const double (&p)[3], float lim) {
  int order = 0;
  double best = INFINITY;
  bool have = false;
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
  return order;
}

template <bool RAW>
__device__ __forceinline__ const double (&icp_side(const double (&p)[3], const double (&d)[3]))[3] {
  if constexpr (RAW) return d;
  else return p;
}
// One pair (landmark i at p, model point `order`) under policy G: the key and index stored, or the pair decided and --
// as far as kept -- added to the columns s.  Every column receives one addition per pair in either case (a dropped
// pair's is +0.0 through a select, never a skipped statement: no sum can become -0.0).
template <class G>
__device__ __forceinline__ void icp_pair(const G& ga, const PoseView& v, int64_t i, int order, const double (&p)[3],
                                         const double* data, const double* model, double (&s)[G::NS],
                                         uint32_t& nkept, uint32_t& nlost) {
  const double y0 = model[3 * order], y1 = model[3 * order + 1], y2 = model[3 * order + 2];
  const double y[3] = {y0, y1, y2};
  if constexpr (G::STORE) {
    const double e0 = p[0] - y0, e1 = p[1] - y1, e2 = p[2] - y2;
    ga.store(v, i, order, trim_key(e0 * e0 + e1 * e1 + e2 * e2));
  } else if constexpr (G::COUNT) {
    const double e0 = p[0] - y0, e1 = p[1] - y1, e2 = p[2] - y2;
    const double dd = e0 * e0 + e1 * e1 + e2 * e2;
    uint8_t code;  // what keep[] receives
    const bool kp = ga.keeps(v, i, order, dd, code, nlost);
    if (ga.keep) ga.keep[i] = code;
    nkept += kp ? 1u : 0u;
    // What the d-side columns sum.  RAW: the landmark is read AGAIN, through a base pointer the compiler cannot see
    // through (it stays in scalar registers) -- held from the first read the landmark would stay live across the search,
    // the pass's register peak, at 6 VGPRs per point
    double d[3];
    if constexpr (G::RAW) {
      const double* again = data;
      asm volatile("" : "+s"(again) : "v"(dd));  // and not before dd is there: p's registers are free by then
#pragma unroll
      for (int r = 0; r < 3; r++) d[r] = again[3 * i + r];
    }
    const double(&x)[3] = icp_side<G::RAW>(p, d);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      s[r] += kp ? x[r] : 0.0;
      s[3 + r] += kp ? y[r] : 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++) s[6 + 3 * r + c] += kp ? x[r] * y[c] : 0.0;
    }
    s[15] += kp ? dd : 0.0;
    if constexpr (G::NS == 18 && G::RAW) {
      s[16] += kp ? x[0] * x[0] : 0.0;
      s[17] += kp ? x[1] * x[1] : 0.0;
    } else if constexpr (G::NS == 18) {
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

// The end of a pass: the workgroup's partial row (pose's slice in `partial`) and its counts
template <int TB, class G>
__device__ __forceinline__ void icp_pass_finish(const G& ga, const double (&s)[G::NS], uint32_t nkept, uint32_t nlost,
                                                double* partial) {
  if constexpr (G::SUMS) block_fold<TB>(s, FoldSum(), partial + (size_t)blockIdx.x * G::NS);
  if constexpr (G::COUNT) block_count<TB>(nkept, ga.pkept + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
  if constexpr (G::LOST) {
    __syncthreads();  // block_count's LDS words are free again
    block_count<TB>(nlost, ga.plost + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
  }
}

// The two search bodies.  Each sits behind one __global__ template (k_icp_pass, k_icp_pass_small) that only forwards
// its arguments: the `__restrict__` parameters of an inlined body give the loads and stores in it alias scopes of their
// own, and the timed ungated kernels are scheduled with those.
template <int TB, int NNMODE, class G>
__device__ __forceinline__ void icp_pass_body(const double* __restrict__ model, const float4* __restrict__ model32,
                                              int nm, const double* __restrict__ data, int64_t nd,
                                              const IcpState* __restrict__ st, double* __restrict__ partial,
                                              int32_t* __restrict__ nn, const NNGrid& ng, const G& ga) {
  constexpr int NS = G::NS;
  st += blockIdx.y;  // the pose's state and partial rows (gridDim.y = 1 outside vcp_icp_multistart)
  partial += (size_t)blockIdx.y * gridDim.x * NS;
  if (st->done) return;
  const PoseView pv = ga.view(st, nd);
  uint32_t nkept = 0, nlost = 0;
  constexpr bool TILED = NNMODE == 1, GRID = NNMODE == 2;
  __shared__ float4 tile[TILED && G::SEARCH ? MTILE : 1];
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
    double p[3];
    trans_point(R, T, d0, d1, d2, p);
    int order = 0;
    if constexpr (!G::SEARCH) {
      order = pv.nn[il];
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
      order = icp_exact_scan(model, model32, nm, q0, q1, q2, p, b1 + tol2);
    }
    }  // !GRID
    if (!live || sub != 0) continue;  // one lane of the group carries the point into the sums
    if constexpr (G::SEARCH && !G::STORE)  // the others keep the index in their own workspace: nn is NULL
      if (nn) nn[i] = order;
    icp_pair(ga, pv, i, order, p, data, model, s, nkept, nlost);
  }
  icp_pass_finish<TB>(ga, s, nkept, nlost, partial);
}

// The two pass kernels: the policy is the last argument; the trimmed and the unique passes get nn = nullptr (their
// own workspace keeps the index found).
template <int TB, int NNMODE, class G>
__global__ __launch_bounds__(TB) void k_icp_pass(const double* __restrict__ model, const float4* __restrict__ model32,
                                                int nm, const double* __restrict__ data, int64_t nd,
                                                const IcpState* __restrict__ st, double* __restrict__ partial,
                                                int32_t* __restrict__ nn, NNGrid ng, G ga) {
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
  constexpr int NS = G::NS;
  st += blockIdx.y;  // the pose's state and partial rows (gridDim.y = 1 outside vcp_icp_multistart)
  partial += (size_t)blockIdx.y * gridDim.x * NS;
  if (st->done) return;
  const PoseView pv = ga.view(st, nd);
  uint32_t nkept = 0, nlost = 0;
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
      trans_point(R, T, d0, d1, d2, p[h]);
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
    if constexpr (G::SEARCH) {
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
    }  // SEARCH
#pragma unroll
    for (int h = 0; h < 2; h++) {
      int order = (int)(__float_as_uint(b1[h]) & imask);
      const bool amb = G::SEARCH && !(b2[h] > b1[h] + tol2[h]);
      if constexpr (!G::SEARCH) order = pv.nn[live[h] ? idx[h] : nd - 1];
      if (amb) order = icp_exact_scan(model, model32, nm, q[h][0], q[h][1], q[h][2], p[h], b1[h] + tol2[h]);
      if (!live[h]) continue;
      if constexpr (G::SEARCH && !G::STORE)  // the others keep the index in their own workspace: nn is NULL
        if (nn) nn[idx[h]] = order;
      icp_pair(ga, pv, idx[h], order, p[h], data, model, s, nkept, nlost);
    }
  }
  icp_pass_finish<TB>(ga, s, nkept, nlost, partial);
}

// Waves per SIMD the pairs kernel of a policy is held to (0: no demand).  AnisoGate: the five of SimGate's kernel, 96
// VGPRs -- left alone its schedule takes 97.
template <class G>
constexpr int PAIRS_WAVES = 0;
template <>
constexpr int PAIRS_WAVES<AnisoGate> = 5;
template <int TB, class G>
__global__ __launch_bounds__(TB, PAIRS_WAVES<G>) void k_icp_pass_small(
    const double* __restrict__ model, const float4* __restrict__ model32, int nm, const double* __restrict__ data,
    int64_t nd, const IcpState* __restrict__ st, double* __restrict__ partial, int32_t* __restrict__ nn, uint32_t imask,
    double tolk, G ga) {
  icp_pass_small_body<TB>(model, model32, nm, data, nd, st, partial, nn, imask, tolk, ga);
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
    vcp_radix_pick(hist[threadIdx.x], p.rank, sh, g, left);
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
    vcp_radix_pick(ghist[(d - 1) * ITPB + threadIdx.x], p.rank, sh, g, left);
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
  vcp_radix_pick(ghist[(TRIM_DIGITS - 1) * ITPB + threadIdx.x], p.rank, sh, g, left);
  trim_push(p, TRIM_DIGITS - 1, g, left);
  if (threadIdx.x == 0) a.sel[h] = TrimSel{((unsigned long long)p.w0 << 32) | p.w1, p.w2, 0u};
  for (int d = 0; d < TRIM_DIGITS; d++) ghist[d * ITPB + threadIdx.x] = 0;
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

// The step of a round that counts its kept pairs (vcp.h, vcp_icp_gated and the forms built on it): the same fold of
// the partial rows, the kept counts of the workgroups added up (integers: exact), then Horn on (sums, kept) and the
// composition -- or, with fewer than min_pairs pairs kept, nothing: R, T and the basis V stay, the round counts and
// `starved` goes up.  Always max_iter rounds, as MODE_VTK.  sums_only: the passes alone (vcp_icp_sums_gated, ...).
// What a form adds to that sits in its FORM type F, the kernel's last argument:
//   NS, LOST         columns of a row; whether the workgroups' lost counts (plost) are added up as well
//   spread(h)        work for the whole workgroup before the totals are read
//   record(h, tot, lost)  thread 0: what the state has no room for, into the pose's side record
//   solve(...)       thread 0: horn(), or what stands in its place
//   SETS             what solve() returns IS the new pose (R, T <- R1, T1); false: it is composed onto the pose
struct GateStepArgs {
  long long min_pairs;
  int max_iter, sums_only;
};
// gated and trimmed rounds: nothing beside the above
struct KeptStep {
  static constexpr int NS = 16;
  static constexpr bool LOST = false, SETS = false;
  const uint32_t* pkept;  // [poses][nb]
  __device__ __forceinline__ void spread(int) const {}
  __device__ __forceinline__ void record(int, const double*, long long) const {}
  __device__ __forceinline__ bool solve(int, const double (&S)[16], long long kept, double R1[9], double T1[3], double* V) const {
    return horn(S, kept, R1, T1, V);
  }
};
// unique-correspondence rounds: the lost counts added up into the pose's side record, and -- reset_L > 0 -- the
// round's slots set back to all ones (uniq_reset)
struct UniqStep : KeptStep {
  static constexpr bool LOST = true;
  const uint32_t* plost;  // [poses][nb]
  long long* lost;        // [poses]
  UniqArgs ua;
  long long reset_L;
  __device__ __forceinline__ void spread(int h) const {
    if (reset_L > 0) uniq_reset(ua, h, reset_L, threadIdx.x, ITPB);
  }
  __device__ __forceinline__ void record(int h, const double*, long long nlost) const { lost[h] = nlost; }
};
// similarity rounds: 18-wide rows, horn_sim in horn's place; the side record holds the two further sums, the product c
// of the factors applied and the count of rounds whose scale was not determined
struct SimSide {
  double s16, s17;  // the last pass's sums[16], sums[17]
  double c;
  int unscaled, pad;
};
struct SimStep : KeptStep {
  static constexpr int NS = 18;
  SimSide* side;  // [poses]
  double ratio_min, ratio_max;
  __device__ __forceinline__ void record(int h, const double* tot, long long) const {
    side[h].s16 = tot[16];
    side[h].s17 = tot[17];
  }
  __device__ __forceinline__ bool solve(int h, const double (&S)[18], long long kept, double R1s[9], double T1[3], double* V) const {
    double ku, cn;
    const int rc = horn_sim(S, kept, side[h].c, ratio_min, ratio_max, R1s, T1, V, &ku, &cn);
    if (rc == 0) return false;
    side[h].c = cn;
    if (rc == 2) side[h].unscaled = side[h].unscaled + 1;
    return true;
  }
};
// anisotropic rounds: 18-wide rows over the raw landmarks, horn_aniso in horn's place, and a step that SETS the pose --
// a small step composed onto R diag(s) would leave that form.  The state's R holds A = R diag(s0, s1, 1), what the pass
// and the score apply; the side record holds the rotation itself, the two scales, their bounds and per axis the count
// of rounds that did not determine it.
struct AnisoSide {
  double s16, s17;  // the last pass's sums[16], sums[17]
  double R[9];
  double s[2], lo[2], hi[2];
  int unscaled[2];
};
struct AnisoStep : KeptStep {
  static constexpr int NS = 18;
  static constexpr bool SETS = true;
  AnisoSide* side;  // [poses]
  __device__ __forceinline__ void record(int h, const double* tot, long long) const {
    side[h].s16 = tot[16];
    side[h].s17 = tot[17];
  }
  __device__ __forceinline__ bool solve(int h, const double (&S)[18], long long kept, double A1[9], double T1[3], double* V) const {
    AnisoSide& sd = side[h];
    double R0[9], Rn[9], sn[2];
    const double s0[2] = {sd.s[0], sd.s[1]}, lo[2] = {sd.lo[0], sd.lo[1]}, hi[2] = {sd.hi[0], sd.hi[1]};
#pragma unroll
    for (int k = 0; k < 9; k++) R0[k] = sd.R[k];
    int det;
    if (!horn_aniso(S, kept, V, R0, s0, lo, hi, Rn, T1, sn, A1, &det)) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) sd.R[k] = Rn[k];
    sd.s[0] = sn[0];
    sd.s[1] = sn[1];
    sd.unscaled[0] = sd.unscaled[0] + ((det & 1) ? 0 : 1);
    sd.unscaled[1] = sd.unscaled[1] + ((det & 2) ? 0 : 1);
    return true;
  }
};
// this workgroup's share of nb counts, added into *total (LDS): integer shuffles and atomics, exact in any order
__device__ __forceinline__ void step_total(const uint32_t* __restrict__ cnt, int nb, unsigned long long* total) {
  unsigned long long c = 0;
  for (int b = threadIdx.x; b < nb; b += ITPB) c += cnt[b];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(total, c);
}
template <class F>
__global__ __launch_bounds__(ITPB) void k_icp_step_kept(const double* __restrict__ partial, int nb,
                                                       IcpState* __restrict__ st, GateStepArgs a, F f) {
  constexpr int NS = F::NS;
  const int h = blockIdx.x;
  st += h;
  partial += (size_t)h * nb * NS;
  if (st->done) return;
  __shared__ double tot[NS];
  __shared__ unsigned long long skept, slost;
  if (threadIdx.x == 0) {
    skept = 0;
    if constexpr (F::LOST) slost = 0;
  }
  icp_fold_rows<ITPB, NS>(partial, nb, st, tot);  // its barrier orders the stores above before the adds below
  step_total(f.pkept + (size_t)h * nb, nb, &skept);
  if constexpr (F::LOST) step_total(f.plost + (size_t)h * nb, nb, &slost);
  f.spread(h);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long kept = (long long)skept;
  st->kept = kept;
  long long lost = 0;
  if constexpr (F::LOST) lost = (long long)slost;
  f.record(h, tot, lost);
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
    double S[NS];
    for (int k = 0; k < NS; k++) S[k] = tot[k];
    double R1[9], T1[3];
    if (!f.solve(h, S, kept, R1, T1, st->V)) {
      st->failed = 1;
      st->done = 1;
      return;
    }
    if constexpr (F::SETS) {
      for (int k = 0; k < 9; k++) st->R[k] = R1[k];
      for (int k = 0; k < 3; k++) st->T[k] = T1[k];
    } else {
      icp_compose(st, R1, T1);
    }
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

// ---- the host side of a run --------------------------------------------------------------------------------------
// The form of a run: which passes and which step a round is made of.  PLAIN (or no variant at all) is the reference /
// VTK / sums-only round of k_icp_pass + k_icp_step; every other kind runs MODE_VTK's fixed round count or
// MODE_SUMS_ONLY with the counted step, on the ungated partition -- and with it the ungated tree of the sums.
//   GATED    the gated pass
//   SIM      the gated pass over 18-wide rows, horn_sim in the step
//   TRIMMED  per round the distance pass, the select, the trimmed sums pass
//   UNIQUE   per round the distance pass, the tie pass, the sums pass, the slots' reset
//   ANISO    the gated pass over 18-wide rows of the raw landmarks, horn_aniso in the step, which sets the pose
enum IcpKind { ICP_PLAIN = 0, ICP_GATED, ICP_SIM, ICP_TRIMMED, ICP_UNIQUE, ICP_ANISO };
struct IcpVariant {
  IcpKind kind;
  const double* sched;  // host, [n_sched], validated by the caller: the gates, or TRIMMED's keep shares (none: m_fixed)
  int n_sched;
  long long min_pairs;
  long long m_fixed;            // TRIMMED: > 0: the keep count itself (vcp_icp_sums_trimmed)
  double ratio_min, ratio_max;  // SIM, ANISO, validated by the caller
  const double* init_scale;     // ANISO: host, [poses][2] or NULL (all 1.0)
  uint8_t* d_keep;              // [nd] or NULL
  // host, [nst]: per pose what the state has no room for -- SimSide (SIM), TrimSel, the last select (TRIMMED), long long,
  // the last round's lost count (UNIQUE), AnisoSide (ANISO)
  void* side_out;
  const void* side_in;  // host, [nst] or NULL (all zero): ANISO's side records at the start
};
size_t icp_side_size(IcpKind k) {
  return k == ICP_SIM       ? sizeof(SimSide)
         : k == ICP_TRIMMED ? sizeof(TrimSel)
         : k == ICP_UNIQUE  ? sizeof(long long)
         : k == ICP_ANISO   ? sizeof(AnisoSide)
                            : 0;
}

// Where everything of a run lies, in bytes from the start of its buffer.
//   b_icp_part  the nst states (icp_states), from the next 256-byte boundary [nst][nb][16 or 18] partial rows; a
//               counted run: then the schedule, [nst][nb] kept counts (UNIQUE: and as many lost counts), the side records
//   b_icpt      TRIMMED and UNIQUE: per (pose, landmark) 8 bytes of key, then 4 of index; from the next 256-byte
//               boundary TRIMMED's select workspace (per pose 12 prefixes, then 12 x 256 counters) or UNIQUE's slots
//               (per (pose, target) 8 bytes of key, then 4 of index)
//   staging     the states, the schedule, the side records
struct IcpLayout {
  size_t rows, sched, pkept, plost, side, part_bytes;
  size_t nn, ws, ws_bytes, icpt_bytes;
  size_t h_sched, h_side, h_bytes;
  size_t side_bytes;
};
size_t icpt_keys_bytes(int nst, int64_t nd) { return ((size_t)nst * (size_t)nd * 12 + 255) & ~(size_t)255; }
int32_t* icpt_nn(vcp_ctx* ctx, int nst, int64_t nd) {
  return reinterpret_cast<int32_t*>(ctx->b_icpt.as<char>() + (size_t)nst * (size_t)nd * 8);
}
IcpLayout icp_layout(const IcpVariant& v, int nst, int nb, int64_t nd, int64_t nm) {
  IcpLayout l{};
  const size_t cnt_bytes = v.kind == ICP_PLAIN ? 0 : ((size_t)nst * nb * sizeof(uint32_t) + 15) & ~(size_t)15;
  l.side_bytes = (size_t)nst * icp_side_size(v.kind);
  l.rows = icp_states_bytes(nst);
  l.sched = l.rows + (size_t)nst * nb * (v.kind == ICP_SIM || v.kind == ICP_ANISO ? 18 : 16) * sizeof(double);
  l.pkept = l.sched + (size_t)v.n_sched * sizeof(double);
  l.plost = l.pkept + cnt_bytes;
  l.side = l.plost + (v.kind == ICP_UNIQUE ? cnt_bytes : 0);
  l.part_bytes = l.side + l.side_bytes;
  if (v.kind == ICP_TRIMMED || v.kind == ICP_UNIQUE) {
    l.nn = (size_t)nst * (size_t)nd * 8;
    l.ws = icpt_keys_bytes(nst, nd);
    l.ws_bytes = v.kind == ICP_TRIMMED ? (size_t)nst * TRIM_DIGITS * (sizeof(TrimPrefix) + ITPB * sizeof(uint32_t))
                                       : (size_t)nst * (size_t)nm * 12;
    l.icpt_bytes = l.ws + l.ws_bytes;
  }
  l.h_sched = (size_t)nst * sizeof(IcpState);
  l.h_side = l.h_sched + (size_t)v.n_sched * sizeof(double);
  l.h_bytes = l.h_side + l.side_bytes;
  return l;
}

// One pass of a run under policy G, on the path (pairs / grid / tiled) and workgroup size the run has chosen.
struct PassLaunch {
  vcp_ctx* ctx;
  bool small, grid, tiled;
  int nb, nst;
  const double* model;
  const float4* model32;
  int nm;
  const double* data;
  int64_t nd;
  IcpState* st;
  double* part;
  NNGrid ng;
  uint32_t imask;
  double tolk;
  template <int TB, int NNMODE, class G>
  int full(int32_t* nn, const G& g) const {
    VCP_LAUNCH(ctx, (k_icp_pass<TB, NNMODE, G>), dim3(nb, nst), dim3(TB), 0, ctx->stream, model, model32, nm, data, nd,
               st, part, nn, ng, g);
    return VCP_OK;
  }
  template <int TB, class G>
  int pairs(int32_t* nn, const G& g) const {
    VCP_LAUNCH(ctx, (k_icp_pass_small<TB, G>), dim3(nb, nst), dim3(TB), 0, ctx->stream, model, model32, nm, data, nd,
               st, part, nn, imask, tolk, g);
    return VCP_OK;
  }
  template <class G>
  int operator()(int32_t* nn, const G& g) const {
    if (grid) return small ? full<64, 2>(nn, g) : full<ITPB, 2>(nn, g);
    if (tiled) return small ? full<64, 1>(nn, g) : full<ITPB, 1>(nn, g);
    return small ? pairs<64>(nn, g) : pairs<ITPB>(nn, g);
  }
};

// Runs rounds on device-resident model/data until the states say done.  `init` carries the starting R,T of nst
// independent states (nst > 1: vcp_icp_multistart, MODE_VTK), `out` receives them.  all_rounds: enqueue every round
// and synchronise once (a fixed round count needs nothing back in between).  ng_out (may be NULL) receives the
// model's grid; ng_out->rec == nullptr when the full scans serve the model.  var: NULL for a PLAIN run.
int icp_run(vcp_ctx* ctx, const double* d_model, int64_t nm, const double* d_data, int64_t nd, const IcpState* init,
            int nst, double tol, int stop_rule, int max_iter, int mode, IcpState* out, int32_t* d_nn, bool all_rounds,
            NNGrid* ng_out, const IcpVariant* var = nullptr) {
  static const IcpVariant plain{};
  const IcpVariant& v = var ? *var : plain;
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
  const IcpLayout lay = icp_layout(v, nst, nb, nd, nm);
  VCP_TRY(vcp_ensure(ctx, ctx->b_icp_part, lay.part_bytes));
  if (lay.icpt_bytes) VCP_TRY(vcp_ensure(ctx, ctx->b_icpt, lay.icpt_bytes));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux0, (size_t)nm * sizeof(float4) + 64));
  char* const dp = ctx->b_icp_part.as<char>();
  char* const dt = lay.icpt_bytes ? ctx->b_icpt.as<char>() : nullptr;
  IcpState* d_st = icp_states(ctx);
  double* part = reinterpret_cast<double*>(dp + lay.rows);
  double* d_sched = reinterpret_cast<double*>(dp + lay.sched);
  uint32_t* pkept = reinterpret_cast<uint32_t*>(dp + lay.pkept);
  uint32_t* plost = reinterpret_cast<uint32_t*>(dp + lay.plost);
  char* d_side = dp + lay.side;
  unsigned long long* d_key = reinterpret_cast<unsigned long long*>(dt);
  int32_t* d_knn = dt ? reinterpret_cast<int32_t*>(dt + lay.nn) : nullptr;
  char* d_ws = dt ? dt + lay.ws : nullptr;
  // a counted run stages its schedule behind the states: the caller's array may be gone before the copy has run
  char* h_base = reinterpret_cast<char*>(nst == 1 && v.kind == ICP_PLAIN ? ctx->pinned : vcp_stage(ctx, lay.h_bytes));
  if (!h_base) return vcp_fail(ctx, VCP_ERR_NOMEM, "pinned staging of %d ICP states", nst);
  IcpState* h_st = reinterpret_cast<IcpState*>(h_base);
  char* h_side = h_base + lay.h_side;
  std::memcpy(h_st, init, (size_t)nst * sizeof(IcpState));
  VCP_HIP(ctx, hipMemcpyAsync(d_st, h_st, (size_t)nst * sizeof(IcpState), hipMemcpyHostToDevice, st));
  if (v.n_sched) {
    std::memcpy(h_base + lay.h_sched, v.sched, (size_t)v.n_sched * sizeof(double));
    VCP_HIP(ctx, hipMemcpyAsync(d_sched, h_base + lay.h_sched, (size_t)v.n_sched * sizeof(double), hipMemcpyHostToDevice, st));
  }
  // what makes the call independent of the context's history
  const bool sel_wg = nd <= TRIM_SELECT_WG_MAX;
  TrimPrefix* d_slot = reinterpret_cast<TrimPrefix*>(d_ws);
  uint32_t* d_ghist = v.kind == ICP_TRIMMED ? reinterpret_cast<uint32_t*>(d_slot + (size_t)nst * TRIM_DIGITS) : nullptr;
  if (v.kind == ICP_SIM) {  // every pose starts at c = 1, no round unscaled
    for (int k = 0; k < nst; k++) reinterpret_cast<SimSide*>(h_side)[k] = SimSide{0.0, 0.0, 1.0, 0, 0};
    VCP_HIP(ctx, hipMemcpyAsync(d_side, h_side, lay.side_bytes, hipMemcpyHostToDevice, st));
  } else if (v.kind == ICP_ANISO) {  // the caller's records: rotation, scales and bounds of every pose
    if (v.side_in) std::memcpy(h_side, v.side_in, lay.side_bytes);
    else std::memset(h_side, 0, lay.side_bytes);
    VCP_HIP(ctx, hipMemcpyAsync(d_side, h_side, lay.side_bytes, hipMemcpyHostToDevice, st));
  } else if (v.kind == ICP_TRIMMED) {
    // the selects' results are read back at the end; the multi-workgroup form's histograms start at zero
    VCP_HIP(ctx, hipMemsetAsync(d_side, 0, lay.side_bytes, st));
    if (!sel_wg) VCP_HIP(ctx, hipMemsetAsync(d_ghist, 0, (size_t)nst * TRIM_DIGITS * ITPB * sizeof(uint32_t), st));
  } else if (v.kind == ICP_UNIQUE) {
    // every slot all ones, once per call: the rounds set back what they touch
    VCP_HIP(ctx, hipMemsetAsync(d_ws, 0xFF, lay.ws_bytes, st));
    VCP_HIP(ctx, hipMemsetAsync(d_side, 0, lay.side_bytes, st));
  }
  const StepArgs sa{(long long)nd, tol, stop_rule, max_iter, mode};
  const GateStepArgs gsa{v.min_pairs, max_iter, mode == MODE_SUMS_ONLY ? 1 : 0};
  const GateArgs ga{d_sched, v.n_sched, pkept, v.d_keep};
  const TrimArgs ta{d_sched, v.n_sched, v.m_fixed, d_key, d_knn, reinterpret_cast<TrimSel*>(d_side), pkept, v.d_keep};
  unsigned long long* skey = reinterpret_cast<unsigned long long*>(d_ws);
  const UniqArgs ua{d_sched, v.n_sched, (int)nm,
                    d_key,   d_knn,     skey,
                    v.kind == ICP_UNIQUE ? reinterpret_cast<uint32_t*>(skey + (size_t)nst * (size_t)nm) : nullptr,
                    pkept,   plost,     v.d_keep};
  const bool reset_in_step = nd <= UNIQ_RESET_STEP_MAX;
  float4* model32 = ctx->b_aux0.as<float4>();
  if (!grid) {  // the binary32 screening frame and copy serve the full scans only
    VCP_LAUNCH(ctx, k_model_frame, dim3(1), dim3(ITPB), 0, st, d_model, nm, d_st, nst);
    VCP_LAUNCH(ctx, k_model32, dim3(vcp_blocks(nm, ITPB)), dim3(ITPB), 0, st, d_model, nm, d_st, model32);
  }
  const PassLaunch pass{ctx, small, grid, tiled, nb, nst, d_model, model32, (int)nm, d_data, nd, d_st, part, ng, imask, tolk};
  const dim3 one_per_pose(nst), threads(ITPB);
  auto all_done = [&]() {
    for (int k = 0; k < nst; k++)
      if (!h_st[k].done) return false;
    return true;
  };
  int launched = 0;
  for (;;) {
    const int batch = mode == MODE_SUMS_ONLY ? 1 : std::min(all_rounds ? max_iter : ICP_BATCH, max_iter - launched);
    for (int b = 0; b < batch; b++) {
      switch (v.kind) {
        case ICP_PLAIN:
          VCP_TRY(pass(d_nn, NoGate()));
          VCP_LAUNCH(ctx, k_icp_step, one_per_pose, threads, 0, st, part, nb, d_st, sa);
          break;
        case ICP_GATED:
          VCP_TRY(pass(d_nn, ga));
          VCP_LAUNCH(ctx, k_icp_step_kept<KeptStep>, one_per_pose, threads, 0, st, part, nb, d_st, gsa, KeptStep{pkept});
          break;
        case ICP_SIM:
          VCP_TRY(pass(d_nn, SimGate{ga}));
          VCP_LAUNCH(ctx, k_icp_step_kept<SimStep>, one_per_pose, threads, 0, st, part, nb, d_st, gsa,
                     (SimStep{{pkept}, reinterpret_cast<SimSide*>(d_side), v.ratio_min, v.ratio_max}));
          break;
        case ICP_ANISO:
          VCP_TRY(pass(d_nn, AnisoGate{ga}));
          VCP_LAUNCH(ctx, k_icp_step_kept<AnisoStep>, one_per_pose, threads, 0, st, part, nb, d_st, gsa,
                     (AnisoStep{{pkept}, reinterpret_cast<AnisoSide*>(d_side)}));
          break;
        case ICP_TRIMMED:  // the pass twice (distances, then sums) with the select between them
          VCP_TRY(pass(nullptr, TrimDist{ta}));
          if (sel_wg) {
            VCP_LAUNCH(ctx, k_icpt_select_wg, one_per_pose, threads, 0, st, d_st, ta, (int)nd);
          } else {
            const unsigned hb = vcp_blocks(nd, TRIM_HIST_KEYS, TRIM_HIST_BLOCKS);
            for (int d = 0; d < TRIM_DIGITS; d++)
              VCP_LAUNCH(ctx, k_icpt_hist, dim3(hb, nst), threads, 0, st, d_st, ta, nd, d_ghist, d_slot, d);
            VCP_LAUNCH(ctx, k_icpt_select_fin, one_per_pose, threads, 0, st, d_st, ta, d_ghist, d_slot);
          }
          VCP_TRY(pass(nullptr, TrimSum{ta}));
          VCP_LAUNCH(ctx, k_icp_step_kept<KeptStep>, one_per_pose, threads, 0, st, part, nb, d_st, gsa, KeptStep{pkept});
          break;
        case ICP_UNIQUE: {  // likewise, with the tie pass between them
          const dim3 tie_grid(vcp_blocks(nd, UNIQ_TIE_KEYS, UNIQ_TIE_BLOCKS), nst);
          VCP_TRY(pass(nullptr, UniqDist{ua}));
          VCP_LAUNCH(ctx, k_icpu_tie, tie_grid, threads, 0, st, d_st, ua, nd);
          VCP_TRY(pass(nullptr, UniqSum{ua}));
          const bool reset = mode != MODE_SUMS_ONLY;  // sums only: one round, nothing left to decide with the slots
          if (reset && !reset_in_step) VCP_LAUNCH(ctx, k_icpu_reset, tie_grid, threads, 0, st, d_st, ua, nd);
          VCP_LAUNCH(ctx, k_icp_step_kept<UniqStep>, one_per_pose, threads, 0, st, part, nb, d_st, gsa,
                     (UniqStep{{pkept}, plost, reinterpret_cast<long long*>(d_side), ua,
                               (long long)(reset && reset_in_step ? nd : 0)}));
          break;
        }
      }
    }
    launched += batch;
    VCP_HIP(ctx, hipMemcpyAsync(h_st, d_st, (size_t)nst * sizeof(IcpState), hipMemcpyDeviceToHost, st));
    if (lay.side_bytes) VCP_HIP(ctx, hipMemcpyAsync(h_side, d_side, lay.side_bytes, hipMemcpyDeviceToHost, st));
    VCP_HIP(ctx, hipStreamSynchronize(st));
    if (all_done() || launched >= max_iter || mode == MODE_SUMS_ONLY) break;
  }
  std::memcpy(out, h_st, (size_t)nst * sizeof(IcpState));
  if (lay.side_bytes) std::memcpy(v.side_out, h_side, lay.side_bytes);
  for (int k = 0; k < nst; k++)
    if (out[k].failed) return vcp_fail(ctx, VCP_ERR_ARG, "Horn solve failed (non-finite sums)%s", nst > 1 ? " in a pose" : "");
  return VCP_OK;
}

// M = [R | T; 0 0 0 1], row major: a state as the VTK-like entry points return it
__host__ __device__ inline void state_to_M(const IcpState& s, double M[16]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) M[4 * r + c] = s.R[3 * r + c];
    M[4 * r + 3] = s.T[r];
  }
  M[12] = M[13] = M[14] = 0;
  M[15] = 1;
}

// The landmarks of the VTK-like entry points: every step-th source point, step = ns / max_landmarks when
// ns > max_landmarks (vtkIterativeClosestPointTransform.h)
std::vector<double> icp_landmarks(const double* source, int64_t ns, int max_landmarks, int64_t* step_o) {
  int64_t step = 1;
  if (ns > max_landmarks) step = ns / max_landmarks;
  const int64_t nb = ns / step;
  std::vector<double> a((size_t)3 * nb);
  for (int64_t i = 0, j = 0; i < nb; i++, j += step)
    for (int c = 0; c < 3; c++) a[3 * i + c] = source[3 * j + c];
  *step_o = step;
  return a;
}
// and the centroid of their centroid start: the sequential binary64 mean over ALL n points
void icp_mean(const double* x, int64_t n, double m[3]) {
  double s[3] = {0, 0, 0};
  for (int64_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) s[c] += x[3 * i + c];
  for (int c = 0; c < 3; c++) m[c] = s[c] / (double)n;
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
  state_to_M(st[h], M);
  bool hit = false;
  if (j < ns) {  // uniform per NNG-lane group: the grid query's shuffles stay within live groups
    double m[3];
    mtc::transform(M, src[3 * j], src[3 * j + 1], src[3 * j + 2], m);
    int best;
    const double bd = mtc::nearest<GRID>(tgt, nt, ng, m, sub, best);
    hit = bd < max_dist && sub == 0;
  }
  __shared__ uint32_t wc[ITPB / 64];
  // (by hand: wave.hpp's block_count changes this kernel's instruction stream, profiles/wave_refactor_codegen.md)
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
  int64_t step;
  const std::vector<double> a = icp_landmarks(source, ns, max_landmarks, &step);
  const int64_t nb = ns / step;
  IcpState init, fin;
  identity(init);
  if (start_by_matching_centroids) {
    double ms[3], mt[3];
    icp_mean(source, ns, ms);
    icp_mean(target, nt, mt);
    for (int c = 0; c < 3; c++) init.T[c] = mt[c] - ms[c];
  }
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)nt * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, (size_t)nb * 24));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, target, (size_t)nt * 24, hipMemcpyHostToDevice, ctx->stream));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, a.data(), (size_t)nb * 24, hipMemcpyHostToDevice, ctx->stream));
  VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `a` is a local buffer
  VCP_TRY(icp_run(ctx, ctx->b_in0.as<double>(), nt, ctx->b_in2.as<double>(), nb, &init, 1, 0.0, VCP_STOP_SSE_DELTA,
                  max_iter, MODE_VTK, &fin, nullptr, false, nullptr));
  state_to_M(fin, M);
  if (mean_dist) *mean_dist = std::sqrt(fin.d / (double)nb);
  if (iters_o) *iters_o = fin.round;
  return VCP_OK;
}

// Multi-start form of vcp_icp_vtklike (vcp.h): the same landmarks, rounds and arithmetic per pose, from H starts at
// once; the target's grid (or screening frame) is built once and serves every pose and the score.
// var says which form runs (PLAIN: vcp_icp_multistart); its schedule and bounds are checked here, next to the other
// arguments.  IcpOutputs: what the counted forms return per pose beside the common outputs; each may be NULL.
struct IcpOutputs {
  int64_t* kept;      // the states' counters
  int32_t* starved;
  double* trim_dist;  // TRIMMED: the root of the last round's thr
  double* ratio;      // SIM: the side records' c
  int32_t* unscaled;  //      and count
  int64_t* lost;      // UNIQUE: the last round's count of pairs that were not their target's winner
  double* scale;       // ANISO: [poses][2] the side records' s
  int32_t* unscaled2;  //        [poses][2] and counts
};
static bool sim_range_ok(double ratio_min, double ratio_max) {
  return ratio_min > 0.0 && ratio_max >= ratio_min && ratio_max <= 1.7976931348623157e308;  // false for NaN
}
static const char* icp_phase(IcpKind k, bool score) {
  static const char* const names[6][2] = {{"icpms_rounds", "icpms_score"},
                                          {"icpg_rounds", "icpg_score"},
                                          {"icps_rounds", "icps_score"},
                                          {"icpt_rounds", "icpt_score"},
                                          {"icpu_rounds", "icpu_score"},
                                          {"icpa_rounds", "icpa_score"}};
  return names[k][score ? 1 : 0];
}
static int icp_multistart_run(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                              int32_t n_poses, const double* init_R, const double* init_T, int max_iter,
                              int max_landmarks, double inlier_dist, double M_best[16], int32_t* best, double* M_all,
                              double* mean_dist, int32_t* inliers, IcpVariant var, const IcpOutputs& o) {
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
  const bool counted = var.kind != ICP_PLAIN, shares = var.kind == ICP_TRIMMED;
  if (counted) {  // the schedule: gates > 0, or keep shares in (0, 1]
    if (var.n_sched < 1 || !var.sched) return vcp_fail(ctx, VCP_ERR_ARG, shares ? "n_keep < 1" : "n_gates < 1");
    if (var.min_pairs < 1) return vcp_fail(ctx, VCP_ERR_ARG, "min_pairs < 1");
    for (int k = 0; k < var.n_sched; k++)
      if (!(var.sched[k] > 0.0) || (shares && !(var.sched[k] <= 1.0)))
        return vcp_fail(ctx, VCP_ERR_ARG, shares ? "keep shares must be in (0, 1]" : "gates must be > 0 (+inf allowed)");
  }
  if (var.kind == ICP_SIM || var.kind == ICP_ANISO) {
    if (!sim_range_ok(var.ratio_min, var.ratio_max))
      return vcp_fail(ctx, VCP_ERR_ARG, "need 0 < ratio_min <= ratio_max < inf");
    if (!(var.ratio_min <= 1.0 && 1.0 <= var.ratio_max))
      return vcp_fail(ctx, VCP_ERR_ARG, "need ratio_min <= 1 <= ratio_max");
  }
  for (int64_t k = 0; k < (int64_t)n_poses * 2 && var.kind == ICP_ANISO && var.init_scale; k++) {
    const double s0 = var.init_scale[k];
    if (!(s0 > 0.0) || !sim_range_ok(var.ratio_min * s0, var.ratio_max * s0))  // false for NaN
      return vcp_fail(ctx, VCP_ERR_ARG, "init_scale must be > 0 and finite, and so must its bounds");
  }
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  vcp_phase(ctx, icp_phase(var.kind, false));
  int64_t step;
  const std::vector<double> a = icp_landmarks(source, ns, max_landmarks, &step);
  const int64_t nb = ns / step;
  // source and target means exactly as vcp_icp_vtklike's centroid start computes them
  double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
  if (!init_T) {
    icp_mean(source, ns, ms);
    icp_mean(target, nt, mt);
  }
  std::vector<IcpState> init((size_t)n_poses), fin((size_t)n_poses);
  std::vector<char> side((size_t)n_poses * icp_side_size(var.kind));
  var.side_out = side.data();
  std::vector<AnisoSide> aside(var.kind == ICP_ANISO ? (size_t)n_poses : 0);
  if (var.kind == ICP_ANISO) var.side_in = aside.data();
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
    if (var.kind == ICP_ANISO) {  // the record keeps the rotation; the state gets A = R diag(s0, s1, 1)
      AnisoSide& sd = aside[h];
      sd = AnisoSide{};
      std::memcpy(sd.R, s.R, sizeof(sd.R));
      for (int a = 0; a < 2; a++) {
        sd.s[a] = var.init_scale ? var.init_scale[2 * (size_t)h + a] : 1.0;
        sd.lo[a] = var.ratio_min * sd.s[a];
        sd.hi[a] = var.ratio_max * sd.s[a];
        for (int i = 0; i < 3; i++) s.R[3 * i + a] = sd.R[3 * i + a] * sd.s[a];
      }
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
                  VCP_STOP_SSE_DELTA, max_iter, MODE_VTK, fin.data(), nullptr, true, &ng, &var));
  // score every pose over ALL source points with vcp_match's arithmetic, on the grid the rounds used (vcp_match bins
  // a target of more than 512 points too, and falls back to the full scan on the same condition)
  vcp_phase(ctx, icp_phase(var.kind, true));
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
  // RMS distance of the pairs the last round summed: all nb landmarks, or the kept ones of a counted run (none: +inf)
  auto mean_of = [&](const IcpState& f) {
    if (!counted) return std::sqrt(f.d / (double)nb);
    return f.kept > 0 ? std::sqrt(f.d / (double)f.kept) : (double)INFINITY;
  };
  const SimSide* sim = reinterpret_cast<const SimSide*>(side.data());
  const TrimSel* sel = reinterpret_cast<const TrimSel*>(side.data());
  const long long* nlost = reinterpret_cast<const long long*>(side.data());
  const AnisoSide* ani = reinterpret_cast<const AnisoSide*>(side.data());
  // most inliers, then the smaller mean distance, then the lower index
  int b = 0;
  for (int h = 0; h < n_poses; h++) {
    const double md = mean_of(fin[h]), mb = mean_of(fin[b]);
    if (h_cnt[h] > h_cnt[b] || (h_cnt[h] == h_cnt[b] && md < mb)) b = h;
    if (M_all) state_to_M(fin[h], M_all + 16 * (size_t)h);
    if (mean_dist) mean_dist[h] = md;
    if (inliers) inliers[h] = (int32_t)h_cnt[h];
    if (o.kept) o.kept[h] = (int64_t)fin[h].kept;
    if (o.starved) o.starved[h] = fin[h].starved;
    if (var.kind == ICP_SIM && o.ratio) o.ratio[h] = sim[h].c;
    if (var.kind == ICP_SIM && o.unscaled) o.unscaled[h] = sim[h].unscaled;
    if (var.kind == ICP_UNIQUE && o.lost) o.lost[h] = (int64_t)nlost[h];
    for (int a = 0; a < 2 && var.kind == ICP_ANISO; a++) {
      if (o.scale) o.scale[2 * (size_t)h + a] = ani[h].s[a];
      if (o.unscaled2) o.unscaled2[2 * (size_t)h + a] = ani[h].unscaled[a];
    }
    if (var.kind == ICP_TRIMMED && o.trim_dist) {
      double thr;
      std::memcpy(&thr, &sel[h].key, sizeof(thr));
      o.trim_dist[h] = std::sqrt(thr);
    }
  }
  state_to_M(fin[b], M_best);
  *best = b;
  return VCP_OK;
}

// A counted variant of the multi-start entry points: the schedule and min_pairs; what else a form needs is set by name.
static IcpVariant icp_variant(IcpKind kind, const double* sched, int32_t n_sched, int32_t min_pairs) {
  IcpVariant v{};
  v.kind = kind;
  v.sched = sched;
  v.n_sched = n_sched;
  v.min_pairs = min_pairs;
  return v;
}

int vcp_icp_multistart(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt,
                       int32_t n_poses, const double* init_R, const double* init_T, int max_iter, int max_landmarks,
                       double inlier_dist, double M_best[16], int32_t* best, double* M_all, double* mean_dist,
                       int32_t* inliers) {
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, IcpVariant{}, IcpOutputs{});
}

// vcp_icp_multistart with a per-round gate on the correspondence distance (vcp.h)
int vcp_icp_gated(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                  const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                  int32_t n_gates, int32_t min_pairs, double inlier_dist, double M_best[16], int32_t* best,
                  double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved) {
  IcpOutputs o{};
  o.kept = kept;
  o.starved = starved;
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, icp_variant(ICP_GATED, gates, n_gates, min_pairs), o);
}

// vcp_icp_multistart with a per-round keep share: every round fits on the closest pairs alone (vcp.h)
int vcp_icp_trimmed(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                    const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* keep,
                    int32_t n_keep, int32_t min_pairs, double inlier_dist, double M_best[16], int32_t* best,
                    double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved,
                    double* trim_dist) {
  IcpOutputs o{};
  o.kept = kept;
  o.starved = starved;
  o.trim_dist = trim_dist;
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, icp_variant(ICP_TRIMMED, keep, n_keep, min_pairs), o);
}

// vcp_icp_gated whose rounds fit one isotropic scale beside the rotation and the translation (vcp.h)
int vcp_icp_sim(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                int32_t n_gates, int32_t min_pairs, double ratio_min, double ratio_max, double inlier_dist,
                double M_best[16], int32_t* best, double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept,
                int32_t* starved, double* ratio, int32_t* unscaled) {
  IcpVariant v = icp_variant(ICP_SIM, gates, n_gates, min_pairs);
  v.ratio_min = ratio_min;
  v.ratio_max = ratio_max;
  IcpOutputs o{};
  o.kept = kept;
  o.starved = starved;
  o.ratio = ratio;
  o.unscaled = unscaled;
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, v, o);
}

// vcp_icp_gated where, of the landmarks that share a nearest target, only the closest enters a round's sums (vcp.h)
int vcp_icp_unique(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                   const double* init_R, const double* init_T, int max_iter, int max_landmarks, const double* gates,
                   int32_t n_gates, int32_t min_pairs, double inlier_dist, double M_best[16], int32_t* best,
                   double* M_all, double* mean_dist, int32_t* inliers, int64_t* kept, int32_t* starved, int64_t* lost) {
  IcpOutputs o{};
  o.kept = kept;
  o.starved = starved;
  o.lost = lost;
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, icp_variant(ICP_UNIQUE, gates, n_gates, min_pairs), o);
}

// vcp_icp_gated whose rounds fit one scale for x and one for y beside the rotation and the translation (vcp.h)
int vcp_icp_aniso(vcp_ctx* ctx, const double* source, int64_t ns, const double* target, int64_t nt, int32_t n_poses,
                  const double* init_R, const double* init_T, const double* init_scale, int max_iter, int max_landmarks,
                  const double* gates, int32_t n_gates, int32_t min_pairs, double ratio_min, double ratio_max,
                  double inlier_dist, double M_best[16], int32_t* best, double* M_all, double* mean_dist,
                  int32_t* inliers, int64_t* kept, int32_t* starved, double* scale, int32_t* unscaled) {
  IcpVariant v = icp_variant(ICP_ANISO, gates, n_gates, min_pairs);
  v.ratio_min = ratio_min;
  v.ratio_max = ratio_max;
  v.init_scale = init_scale;
  IcpOutputs o{};
  o.kept = kept;
  o.starved = starved;
  o.scale = scale;
  o.unscaled2 = unscaled;
  return icp_multistart_run(ctx, source, ns, target, nt, n_poses, init_R, init_T, max_iter, max_landmarks, inlier_dist,
                            M_best, best, M_all, mean_dist, inliers, v, o);
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

// Host-side run of the anisotropic step (horn_aniso is __host__ __device__ too).  Returns 1, or 0 where the solve fails.
int vcp_selftest_horn_aniso(const double sums[18], int64_t n, double V[16], int use_v, const double R[9],
                            const double s[2], const double lo[2], const double hi[2], double R_new[9],
                            double T_new[3], double s_new[2], int32_t* determined) {
  if (!sums || !R || !s || !lo || !hi || !R_new || !T_new || !s_new || !determined || n <= 0 || (use_v && !V))
    return VCP_ERR_ARG;
  for (int a = 0; a < 2; a++)
    if (!(s[a] > 0.0) || !sim_range_ok(lo[a], hi[a])) return VCP_ERR_ARG;
  double S[18], Rn[9], Tn[3], sn[2], An[9];
  for (int k = 0; k < 18; k++) S[k] = sums[k];
  int det;
  if (!horn_aniso(S, (long long)n, use_v ? V : nullptr, R, s, lo, hi, Rn, Tn, sn, An, &det)) return 0;
  std::memcpy(R_new, Rn, sizeof(Rn));
  std::memcpy(T_new, Tn, sizeof(Tn));
  std::memcpy(s_new, sn, sizeof(sn));
  *determined = det;
  return 1;
}

// One round's passes from (R, T), behind vcp_icp_sums and its forms.  kind says which form; gate serves GATED, SIM (sums
// [18]) and UNIQUE, m serves TRIMMED.  SumsOutputs: the verdicts a form returns beside the sums and nn.
struct SumsOutputs {
  int64_t* kept;   // GATED, SIM, UNIQUE
  uint8_t* keep;   // all but PLAIN; may be NULL
  double* thr_dd;  // TRIMMED
  int64_t* lost;   // UNIQUE
};
static int icp_sums_run(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                        const double T[3], double* sums, int32_t* nn, IcpKind kind, double gate, int64_t m,
                        const SumsOutputs& o) {
  const bool gated = kind == ICP_GATED || kind == ICP_SIM || kind == ICP_UNIQUE || kind == ICP_ANISO;
  const bool trimmed = kind == ICP_TRIMMED;
  const bool stored_nn = trimmed || kind == ICP_UNIQUE;  // the rounds that keep the index found in their own workspace
  if (!ctx) return VCP_ERR_ARG;
  if (nm <= 0) return vcp_fail(ctx, VCP_ERR_EMPTY, "empty model");
  if (nd <= 0 || !model || !data || !sums) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (nm >= 0x7FFFFFFFLL / 3) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "model too large");
  if (gated && !(gate > 0.0)) return vcp_fail(ctx, VCP_ERR_ARG, "gate must be > 0 (+inf allowed)");
  if (gated && !o.kept) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (trimmed && !o.thr_dd) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (trimmed && (m < 1 || m > nd)) return vcp_fail(ctx, VCP_ERR_ARG, "m must be in [1, nd]");
  if (stored_nn && nd > 0xFFFFFFFFLL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "the key holds the landmark in 32 bits");
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)nm * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_in2, (size_t)nd * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, (size_t)nd * 4));
  if (o.keep) VCP_TRY(vcp_ensure(ctx, ctx->b_out1, (size_t)nd));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, model, (size_t)nm * 24, hipMemcpyHostToDevice, ctx->stream));
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in2.p, data, (size_t)nd * 24, hipMemcpyHostToDevice, ctx->stream));
  IcpState init, fin;
  identity(init);
  if (R) std::memcpy(init.R, R, sizeof(init.R));
  if (T) std::memcpy(init.T, T, sizeof(init.T));
  union {
    SimSide sim;
    TrimSel sel;
    long long lost;
    AnisoSide ani;
  } side{};
  IcpVariant v{};
  v.kind = kind;
  v.min_pairs = 1;
  v.d_keep = o.keep ? ctx->b_out1.as<uint8_t>() : nullptr;
  v.side_out = &side;
  if (gated) {
    v.sched = &gate;
    v.n_sched = 1;
  }
  if (trimmed) v.m_fixed = (long long)m;
  v.ratio_min = v.ratio_max = 1.0;
  VCP_TRY(icp_run(ctx, ctx->b_in0.as<double>(), nm, ctx->b_in2.as<double>(), nd, &init, 1, 0.0, VCP_STOP_SSE_DELTA, 1,
                  MODE_SUMS_ONLY, &fin, nn && !stored_nn ? ctx->b_out0.as<int32_t>() : nullptr, false, nullptr, &v));
  std::memcpy(sums, fin.sums, sizeof(fin.sums));
  if (kind == ICP_SIM) {
    sums[16] = side.sim.s16;
    sums[17] = side.sim.s17;
  }
  if (kind == ICP_ANISO) {
    sums[16] = side.ani.s16;
    sums[17] = side.ani.s17;
  }
  if (gated) *o.kept = (int64_t)fin.kept;
  if (kind == ICP_UNIQUE) *o.lost = (int64_t)side.lost;
  if (trimmed) std::memcpy(o.thr_dd, &side.sel.key, sizeof(double));
  if (nn) {
    const void* d_nn = stored_nn ? (const void*)icpt_nn(ctx, 1, nd) : ctx->b_out0.p;
    VCP_HIP(ctx, hipMemcpyAsync(nn, d_nn, (size_t)nd * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (o.keep) VCP_HIP(ctx, hipMemcpyAsync(o.keep, ctx->b_out1.p, (size_t)nd, hipMemcpyDeviceToHost, ctx->stream));
  if (nn || o.keep) VCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VCP_OK;
}

int vcp_icp_sums(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                 const double T[3], double sums[16], int32_t* nn) {
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, ICP_PLAIN, 0.0, 0, SumsOutputs{});
}

int vcp_icp_sums_gated(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                       const double T[3], double gate, double sums[16], int64_t* kept, int32_t* nn, uint8_t* keep) {
  SumsOutputs o{};
  o.kept = kept;
  o.keep = keep;
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, ICP_GATED, gate, 0, o);
}

int vcp_icp_sums_sim(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                     const double T[3], double gate, double sums[18], int64_t* kept, int32_t* nn, uint8_t* keep) {
  SumsOutputs o{};
  o.kept = kept;
  o.keep = keep;
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, ICP_SIM, gate, 0, o);
}

int vcp_icp_sums_aniso(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double A[9],
                       const double T[3], double gate, double sums[18], int64_t* kept, int32_t* nn, uint8_t* keep) {
  SumsOutputs o{};
  o.kept = kept;
  o.keep = keep;
  return icp_sums_run(ctx, model, nm, data, nd, A, T, sums, nn, ICP_ANISO, gate, 0, o);
}

int vcp_icp_sums_unique(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd, const double R[9],
                        const double T[3], double gate, double sums[16], int64_t* kept, int32_t* nn, uint8_t* keep,
                        int64_t* lost) {
  if (ctx && !lost) return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  SumsOutputs o{};
  o.kept = kept;
  o.keep = keep;
  o.lost = lost;
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, ICP_UNIQUE, gate, 0, o);
}

int vcp_icp_sums_trimmed(vcp_ctx* ctx, const double* model, int64_t nm, const double* data, int64_t nd,
                         const double R[9], const double T[3], int64_t m, double sums[16], double* thr_dd, int32_t* nn,
                         uint8_t* keep) {
  SumsOutputs o{};
  o.keep = keep;
  o.thr_dd = thr_dd;
  return icp_sums_run(ctx, model, nm, data, nd, R, T, sums, nn, ICP_TRIMMED, 0.0, m, o);
}

}  // extern "C"
