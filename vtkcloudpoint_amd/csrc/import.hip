// import.hip -- MainForm.AddFolder's per-row work for scan points on MI355X:
// the Distance filter (FrmMain.cs:1011), the spherical -> Cartesian conversion (:1025-1062) and the exact
// duplicate removal (:1063-1068), which in the C# is an O(n^2) FindAll over everything kept so far.
//
// Here: one conversion pass, then a device hash table on the exact (tmpx, tmpy, tmpz) triple -- insert with
// CAS + atomicMin (a slot ends up holding the smallest row index of its class), second pass keeps a row iff it
// is that smallest index, i.e. the first occurrence, exactly what the sequential FindAll rule keeps.
// Equality is the C#'s `==` on doubles (-0 == +0, NaN != NaN).  sin/cos are the device libm's: tmpx, tmpy are held to
// 2 L + 1 and tmpz to L + 0.5 units of 2^-52 of the true value at the binary64 angles (tests/test_import_accuracy_gpu.py,
// DESIGN.md section 13 for L and the measured figures; the order of operations in the two angle expressions is part of
// that contract), duplicate decisions are bit-exact (identical inputs give identical outputs on either side).
// The duplicate test of the C# compares the STORED, direction-mapped p.X, p.Y with the unmapped tmpx, tmpy
// (:1065); they coincide for the ImportPts defaults xdir = 2, ydir = 1 (ImportPts.cs:18-19).  For other
// directions the C# test can only fire on mirrored points; that quirk is not rebuilt: VCP_ERR_UNSUPPORTED.
#include <cmath>

#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int IT = 256;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;

struct ImpP {
  double x_angle, y_angle;
  int xdir, ydir;
};

__global__ __launch_bounds__(IT) void k_import_convert(const double* __restrict__ rows, int64_t n, ImpP P,
                                                      double* __restrict__ xyz, double* __restrict__ q,
                                                      uint8_t* __restrict__ state) {
  int64_t i = (int64_t)blockIdx.x * IT + threadIdx.x;
  if (i >= n) return;
  const double mx = rows[3 * i], my = rows[3 * i + 1], D = rows[3 * i + 2];
  double X = 0, Y = 0, Z = 0, tx = 0, ty = 0, tz = 0;
  uint8_t st = 0;
  if (!(D == 0 || D > 1000)) {  // FrmMain.cs:1011
    const double PI = 3.14159265358979323846;
    const double yangjiao = (-2) * (mx - P.x_angle) / 180 * PI;
    const double fangweijiao = 2 * (my - P.y_angle) / 180 * PI;
    tx = D * cos(yangjiao) * sin(fangweijiao);
    ty = D * sin(yangjiao) * cos(fangweijiao);
    tz = D * cos(yangjiao);
    const double pick[5] = {0, ty, tx, -ty, -tx};
    X = pick[P.xdir];
    Y = pick[P.ydir];
    Z = tz;
    st = 1;
  }
  xyz[3 * i] = X;
  xyz[3 * i + 1] = Y;
  xyz[3 * i + 2] = Z;
  if (q) {
    q[3 * i] = tx;
    q[3 * i + 1] = ty;
    q[3 * i + 2] = tz;
  }
  state[i] = st;
}

__device__ __forceinline__ uint64_t hash3(double a, double b, double c) {
  uint64_t h = 1469598103934665603ull;
  const double v[3] = {a == 0 ? 0.0 : a, b == 0 ? 0.0 : b, c == 0 ? 0.0 : c};  // -0 and +0 are one class
#pragma unroll
  for (int k = 0; k < 3; k++) {
    h = (h ^ (uint64_t)__double_as_longlong(v[k])) * 1099511628211ull;
    h ^= h >> 29;
  }
  return h;
}
__device__ __forceinline__ bool same3(const double* __restrict__ q, uint32_t a, const double* t) {
  return q[3 * (size_t)a] == t[0] && q[3 * (size_t)a + 1] == t[1] && q[3 * (size_t)a + 2] == t[2];
}

__global__ __launch_bounds__(IT) void k_import_insert(const double* __restrict__ q, const uint8_t* __restrict__ state,
                                                     int64_t n, uint32_t* __restrict__ table, uint32_t mask) {
  int64_t i = (int64_t)blockIdx.x * IT + threadIdx.x;
  if (i >= n || state[i] == 0) return;
  const double t[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
  if (!(t[0] == t[0] && t[1] == t[1] && t[2] == t[2])) return;  // NaN: equal to nothing, never a duplicate
  uint32_t sl = (uint32_t)hash3(t[0], t[1], t[2]) & mask;
  for (;;) {
    uint32_t cur = __hip_atomic_load(&table[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == EMPTY) {
      cur = atomicCAS(&table[sl], EMPTY, (uint32_t)i);
      if (cur == EMPTY) return;  // claimed the slot for this class
    }
    if (same3(q, cur, t)) {  // the slot belongs to my class (any member has the same triple)
      atomicMin(&table[sl], (uint32_t)i);
      return;
    }
    sl = (sl + 1) & mask;
  }
}

__global__ __launch_bounds__(IT) void k_import_mark(const double* __restrict__ q, uint8_t* __restrict__ state, int64_t n,
                                                   const uint32_t* __restrict__ table, uint32_t mask,
                                                   unsigned long long* __restrict__ counters) {
  int64_t i = (int64_t)blockIdx.x * IT + threadIdx.x;
  unsigned kept = 0, dup = 0;
  if (i < n && state[i] != 0) {
    const double t[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    bool isdup = false;
    if (t[0] == t[0] && t[1] == t[1] && t[2] == t[2]) {
      uint32_t sl = (uint32_t)hash3(t[0], t[1], t[2]) & mask;
      for (;;) {
        const uint32_t cur = table[sl];
        if (cur == EMPTY) break;
        if (same3(q, cur, t)) {
          isdup = cur != (uint32_t)i;  // the class keeps its first (smallest-index) row
          break;
        }
        sl = (sl + 1) & mask;
      }
    }
    state[i] = isdup ? 2 : 1;
    kept = !isdup;
    dup = isdup;
  }
  __shared__ uint32_t wc[2 * IT / 64];
  uint32_t a, b;
  if (block_count<IT>(kept, dup, wc, a, b)) {
    if (a) atomicAdd(&counters[2 * (blockIdx.x & 15)], (unsigned long long)a);
    if (b) atomicAdd(&counters[2 * (blockIdx.x & 15) + 1], (unsigned long long)b);
  }
}

// ---- vcp_import_compact: the same conversion, classes keyed by (group, triple) with a count, a stable compaction ----
// The table has `cap` entries of two words: [2 s] the smallest row index of the class that owns slot s (EMPTY: free),
// [2 s + 1] the number of rows of that class.  Both words sit in one 8-byte entry, so a row's atomicMin and atomicAdd go to
// the same sector.  A slot never changes its class: the first row to claim it decides the class, later rows only lower
// the index.  A row whose triple holds a NaN claims a slot like any other and equals nobody (same3 is the C#'s `==`), so
// it is a class of one; its row index goes into its hash, or a million equal NaN rows would probe one run of slots.
__device__ __forceinline__ uint64_t hash_class(const double* t, int32_t g, bool nan, uint32_t i) {
  uint64_t h = hash3(t[0], t[1], t[2]);
  h = (h ^ (uint64_t)(uint32_t)g ^ (nan ? (uint64_t)i << 32 | i : 0)) * 1099511628211ull;
  return h ^ (h >> 29);
}

__global__ __launch_bounds__(IT) void k_impc_clear(uint2* __restrict__ table, uint64_t cap) {
  for (uint64_t s = (uint64_t)blockIdx.x * IT + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * IT)
    table[s] = make_uint2(EMPTY, 0u);
}

__global__ __launch_bounds__(IT) void k_impc_insert(const double* __restrict__ q, const uint8_t* __restrict__ state,
                                                   const int32_t* __restrict__ group, int64_t n,
                                                   uint32_t* __restrict__ table, uint32_t mask,
                                                   uint32_t* __restrict__ slot) {
  int64_t i = (int64_t)blockIdx.x * IT + threadIdx.x;
  if (i >= n || state[i] == 0) return;  // slot[i] of a filtered row is never read
  const double t[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
  const bool nan = !(t[0] == t[0] && t[1] == t[1] && t[2] == t[2]);
  const int32_t g = group ? group[i] : 0;
  uint32_t sl = (uint32_t)hash_class(t, g, nan, (uint32_t)i) & mask;
  for (;;) {
    uint32_t cur = __hip_atomic_load(&table[2 * (size_t)sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == EMPTY) {
      cur = atomicCAS(&table[2 * (size_t)sl], EMPTY, (uint32_t)i);
      if (cur == EMPTY) break;  // claimed the slot for this class
    }
    if ((!group || group[cur] == g) && same3(q, cur, t)) {  // the slot belongs to my class (any member will do)
      atomicMin(&table[2 * (size_t)sl], (uint32_t)i);
      break;
    }
    sl = (sl + 1) & mask;
  }
  atomicAdd(&table[2 * (size_t)sl + 1], 1u);
  slot[i] = sl;
}

// keep[i] = 1 iff row i is unfiltered and the smallest index of its class (slot == NULL: every row is its own class);
// counters[0..15] add up to the number of unfiltered rows
__global__ __launch_bounds__(IT) void k_impc_flag(const uint8_t* __restrict__ state, const uint32_t* __restrict__ slot,
                                                 const uint32_t* __restrict__ table, int64_t n,
                                                 uint32_t* __restrict__ keep, unsigned long long* __restrict__ counters) {
  int64_t i = (int64_t)blockIdx.x * IT + threadIdx.x;
  const bool unf = i < n && state[i] != 0;
  if (i < n) keep[i] = unf && (!slot || table[2 * (size_t)slot[i]] == (uint32_t)i);
  __shared__ uint32_t wc[IT / 64];
  uint32_t a;
  if (block_count<IT>(unf, wc, a) && a) atomicAdd(&counters[blockIdx.x & 15], (unsigned long long)a);
}

struct ImpcOut {
  double *motor, *xyz, *dist;
  int32_t *src, *count, *group_out, *row_to;
};

// pos = the exclusive scan of keep.  Kept rows are written in input order, so the kept lanes of a wave store to
// consecutive entries of every output array.
__global__ __launch_bounds__(IT) void k_impc_scatter(const double* __restrict__ rows, const int32_t* __restrict__ group,
                                                    const double* __restrict__ xyz, const uint8_t* __restrict__ state,
                                                    const uint32_t* __restrict__ slot, const uint32_t* __restrict__ table,
                                                    const uint32_t* __restrict__ pos, int64_t n, ImpcOut o) {
  int64_t i = (int64_t)blockIdx.x * IT + threadIdx.x;
  if (i >= n) return;
  if (state[i] == 0) {
    if (o.row_to) o.row_to[i] = -1;
    return;
  }
  const uint2 e = slot ? reinterpret_cast<const uint2*>(table)[slot[i]] : make_uint2((uint32_t)i, 1u);
  const uint32_t p = pos[e.x];
  if (o.row_to) o.row_to[i] = (int32_t)p;
  if (e.x != (uint32_t)i) return;
  if (o.src) o.src[p] = (int32_t)i;
  if (o.motor) {
    o.motor[2 * (size_t)p] = rows[3 * i];
    o.motor[2 * (size_t)p + 1] = rows[3 * i + 1];
  }
  if (o.dist) o.dist[p] = rows[3 * i + 2];
  if (o.xyz) {
    o.xyz[3 * (size_t)p] = xyz[3 * i];
    o.xyz[3 * (size_t)p + 1] = xyz[3 * i + 1];
    o.xyz[3 * (size_t)p + 2] = xyz[3 * i + 2];
  }
  if (o.count) o.count[p] = (int32_t)e.y;
  if (o.group_out) o.group_out[p] = group ? group[i] : 0;
}

// the argument errors of both forms of vcp_import_compact; VCP_OK when the call can go on
int impc_check(vcp_ctx* ctx, const void* rows, int64_t n, int xdir, int ydir, int dedupe, const void* m) {
  if (!m || n < 0 || xdir < 1 || xdir > 4 || ydir < 1 || ydir > 4 || (n > 0 && !rows))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (dedupe && !(xdir == 2 && ydir == 1))
    return vcp_fail(ctx, VCP_ERR_UNSUPPORTED,
                    "duplicate removal is built for the default directions xdir=2, ydir=1 (FrmMain.cs:1065 compares the "
                    "mapped X,Y with the unmapped tmpx,tmpy)");
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  return VCP_OK;
}
}  // namespace

extern "C" int vcp_import_convert(vcp_ctx* ctx, const double* rows, int64_t n, double x_angle, double y_angle, int xdir,
                                  int ydir, int dedupe, double* xyz, uint8_t* state, int64_t* kept, int64_t* duplicates) {
  if (!ctx) return VCP_ERR_ARG;
  if (n < 0 || xdir < 1 || xdir > 4 || ydir < 1 || ydir > 4 || (n > 0 && (!rows || !xyz || !state)))
    return vcp_fail(ctx, VCP_ERR_ARG, "bad argument");
  if (dedupe && !(xdir == 2 && ydir == 1))
    return vcp_fail(ctx, VCP_ERR_UNSUPPORTED,
                    "duplicate removal is built for the default directions xdir=2, ydir=1 (FrmMain.cs:1065 compares the "
                    "mapped X,Y with the unmapped tmpx,tmpy)");
  if (kept) *kept = 0;
  if (duplicates) *duplicates = 0;
  if (n == 0) return VCP_OK;
  if (n >= 0x7FFFFFF0LL) return vcp_fail(ctx, VCP_ERR_TOO_LARGE, "n beyond 32-bit indexing");
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  uint64_t cap = 1;
  while (cap < (uint64_t)(2 * n + 16)) cap <<= 1;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, (size_t)n * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, (size_t)n * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out1, (size_t)n));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out2, 64 * 8));
  if (dedupe) {
    VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, (size_t)n * 24));
    VCP_TRY(vcp_ensure(ctx, ctx->b_aux1, (size_t)cap * 4));
  }
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, rows, (size_t)n * 24, hipMemcpyHostToDevice, st));
  ImpP P{x_angle, y_angle, xdir, ydir};
  double* q = dedupe ? ctx->b_aux4.as<double>() : nullptr;
  const unsigned nb = vcp_blocks(n, IT);
  VCP_LAUNCH(ctx, k_import_convert, dim3(nb), dim3(IT), 0, st, ctx->b_in0.as<double>(), n, P, ctx->b_out0.as<double>(),
                  q, ctx->b_out1.as<uint8_t>());
  unsigned long long* counters = ctx->b_out2.as<unsigned long long>();
  VCP_HIP(ctx, hipMemsetAsync(counters, 0, 64 * 8, st));
  if (dedupe) {
    uint32_t* table = ctx->b_aux1.as<uint32_t>();
    VCP_HIP(ctx, hipMemsetAsync(table, 0xFF, (size_t)cap * 4, st));
    VCP_LAUNCH(ctx, k_import_insert, dim3(nb), dim3(IT), 0, st, q, ctx->b_out1.as<uint8_t>(), n, table,
                    (uint32_t)(cap - 1));
    VCP_LAUNCH(ctx, k_import_mark, dim3(nb), dim3(IT), 0, st, q, ctx->b_out1.as<uint8_t>(), n, table,
                    (uint32_t)(cap - 1), counters);
  }
  unsigned long long* hp = reinterpret_cast<unsigned long long*>(ctx->pinned);
  VCP_HIP(ctx, hipMemcpyAsync(xyz, ctx->b_out0.p, (size_t)n * 24, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(state, ctx->b_out1.p, (size_t)n, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipMemcpyAsync(hp, counters, 32 * 8, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  int64_t k = 0, d = 0;
  if (dedupe) {
    for (int b = 0; b < 16; b++) {
      k += (int64_t)hp[2 * b];
      d += (int64_t)hp[2 * b + 1];
    }
  } else {
    for (int64_t i = 0; i < n; i++) k += state[i] != 0;
  }
  if (kept) *kept = k;
  if (duplicates) *duplicates = d;
  return VCP_OK;
}

extern "C" int vcp_import_compact_dev(vcp_ctx* ctx, const double* d_rows, int64_t n, const int32_t* d_group, double x_angle,
                                      double y_angle, int xdir, int ydir, int dedupe, double* d_motor, double* d_xyz,
                                      double* d_dist, int32_t* d_src, int32_t* d_count, int32_t* d_group_out,
                                      int32_t* d_row_to, int64_t* m, int64_t* duplicates) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(impc_check(ctx, d_rows, n, xdir, ydir, dedupe, m));
  VCP_TRY(vcp_bind(ctx));
  vcp_phase_reset(ctx);
  if (n == 0) {
    ctx->last_timing.clear();
    *m = 0;
    if (duplicates) *duplicates = 0;
    return VCP_OK;
  }
  hipStream_t st = ctx->stream;
  uint64_t cap = 1;
  while (cap < (uint64_t)(2 * n + 16)) cap <<= 1;
  const size_t nn = (size_t)n;
  VCP_TRY(vcp_ensure(ctx, ctx->b_out0, nn * 24));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out1, nn));
  VCP_TRY(vcp_ensure(ctx, ctx->b_out2, 64 * 8));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux2, nn * 4));
  if (dedupe) {
    VCP_TRY(vcp_ensure(ctx, ctx->b_aux4, nn * 24));
    VCP_TRY(vcp_ensure(ctx, ctx->b_aux1, (size_t)cap * 8));
    VCP_TRY(vcp_ensure(ctx, ctx->b_aux0, nn * 4));
  }
  double* xyz = ctx->b_out0.as<double>();
  uint8_t* state = ctx->b_out1.as<uint8_t>();
  unsigned long long* counters = ctx->b_out2.as<unsigned long long>();  // [16] unfiltered rows, then the scan's total
  uint32_t* d_total = reinterpret_cast<uint32_t*>(counters + 16);
  uint32_t* keep = ctx->b_aux2.as<uint32_t>();
  double* q = dedupe ? ctx->b_aux4.as<double>() : nullptr;
  uint32_t* table = dedupe ? ctx->b_aux1.as<uint32_t>() : nullptr;
  uint32_t* slot = dedupe ? ctx->b_aux0.as<uint32_t>() : nullptr;
  const unsigned nb = vcp_blocks(n, IT);

  vcp_phase(ctx, "impc_convert");
  VCP_HIP(ctx, hipMemsetAsync(counters, 0, 64 * 8, st));
  ImpP P{x_angle, y_angle, xdir, ydir};
  VCP_LAUNCH(ctx, k_import_convert, dim3(nb), dim3(IT), 0, st, d_rows, n, P, xyz, q, state);

  vcp_phase(ctx, "impc_dedupe");
  if (dedupe) {
    VCP_LAUNCH(ctx, k_impc_clear, dim3(vcp_blocks((int64_t)cap, IT, 1 << 20)), dim3(IT), 0, st, reinterpret_cast<uint2*>(table),
               cap);
    VCP_LAUNCH(ctx, k_impc_insert, dim3(nb), dim3(IT), 0, st, q, state, d_group, n, table, (uint32_t)(cap - 1), slot);
  }

  vcp_phase(ctx, "impc_compact");
  VCP_LAUNCH(ctx, k_impc_flag, dim3(nb), dim3(IT), 0, st, state, slot, table, n, keep, counters);
  VCP_TRY(vcp_exclusive_scan_u32(ctx, keep, keep, n, d_total));
  ImpcOut o{d_motor, d_xyz, d_dist, d_src, d_count, d_group_out, d_row_to};
  VCP_LAUNCH(ctx, k_impc_scatter, dim3(nb), dim3(IT), 0, st, d_rows, d_group, xyz, state, slot, table, keep, n, o);
  unsigned long long* hp = reinterpret_cast<unsigned long long*>(ctx->pinned);
  VCP_HIP(ctx, hipMemcpyAsync(hp, counters, 17 * 8, hipMemcpyDeviceToHost, st));
  VCP_TRY(vcp_phase_finish(ctx));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  int64_t unfiltered = 0;
  for (int b = 0; b < 16; b++) unfiltered += (int64_t)hp[b];
  const int64_t kept = (int64_t)(uint32_t)hp[16];
  *m = kept;
  if (duplicates) *duplicates = unfiltered - kept;
  return VCP_OK;
}

extern "C" int vcp_import_compact(vcp_ctx* ctx, const double* rows, int64_t n, const int32_t* group, double x_angle,
                                  double y_angle, int xdir, int ydir, int dedupe, double* motor, double* xyz, double* dist,
                                  int32_t* src, int32_t* count, int32_t* group_out, int32_t* row_to, int64_t* m,
                                  int64_t* duplicates) {
  if (!ctx) return VCP_ERR_ARG;
  VCP_TRY(impc_check(ctx, rows, n, xdir, ydir, dedupe, m));
  if (n == 0)  // no copies: the device form's answer
    return vcp_import_compact_dev(ctx, nullptr, 0, nullptr, x_angle, y_angle, xdir, ydir, dedupe, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, m, duplicates);
  VCP_TRY(vcp_bind(ctx));
  hipStream_t st = ctx->stream;
  // out: [motor n*16 | xyz n*24 | dist n*8 | src n*4 | count n*4 | group_out n*4 | row_to n*4]
  const size_t nn = (size_t)n;
  const size_t o_xyz = nn * 16, o_dist = o_xyz + nn * 24, o_src = o_dist + nn * 8, o_count = o_src + nn * 4,
               o_group = o_count + nn * 4, o_to = o_group + nn * 4;
  VCP_TRY(vcp_ensure(ctx, ctx->b_in0, nn * 24));
  if (group) VCP_TRY(vcp_ensure(ctx, ctx->b_in1, nn * 4));
  VCP_TRY(vcp_ensure(ctx, ctx->b_aux3, o_to + nn * 4));
  char* dout = ctx->b_aux3.as<char>();
  VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in0.p, rows, nn * 24, hipMemcpyHostToDevice, st));
  if (group) VCP_HIP(ctx, hipMemcpyAsync(ctx->b_in1.p, group, nn * 4, hipMemcpyHostToDevice, st));
  int64_t k = 0, d = 0;
  VCP_TRY(vcp_import_compact_dev(
      ctx, ctx->b_in0.as<double>(), n, group ? ctx->b_in1.as<int32_t>() : nullptr, x_angle, y_angle, xdir, ydir, dedupe,
      motor ? reinterpret_cast<double*>(dout) : nullptr, xyz ? reinterpret_cast<double*>(dout + o_xyz) : nullptr,
      dist ? reinterpret_cast<double*>(dout + o_dist) : nullptr, src ? reinterpret_cast<int32_t*>(dout + o_src) : nullptr,
      count ? reinterpret_cast<int32_t*>(dout + o_count) : nullptr,
      group_out ? reinterpret_cast<int32_t*>(dout + o_group) : nullptr,
      row_to ? reinterpret_cast<int32_t*>(dout + o_to) : nullptr, &k, &d));
  const size_t kk = (size_t)k;
  if (motor && kk) VCP_HIP(ctx, hipMemcpyAsync(motor, dout, kk * 16, hipMemcpyDeviceToHost, st));
  if (xyz && kk) VCP_HIP(ctx, hipMemcpyAsync(xyz, dout + o_xyz, kk * 24, hipMemcpyDeviceToHost, st));
  if (dist && kk) VCP_HIP(ctx, hipMemcpyAsync(dist, dout + o_dist, kk * 8, hipMemcpyDeviceToHost, st));
  if (src && kk) VCP_HIP(ctx, hipMemcpyAsync(src, dout + o_src, kk * 4, hipMemcpyDeviceToHost, st));
  if (count && kk) VCP_HIP(ctx, hipMemcpyAsync(count, dout + o_count, kk * 4, hipMemcpyDeviceToHost, st));
  if (group_out && kk) VCP_HIP(ctx, hipMemcpyAsync(group_out, dout + o_group, kk * 4, hipMemcpyDeviceToHost, st));
  if (row_to) VCP_HIP(ctx, hipMemcpyAsync(row_to, dout + o_to, nn * 4, hipMemcpyDeviceToHost, st));
  VCP_HIP(ctx, hipStreamSynchronize(st));
  *m = k;
  if (duplicates) *duplicates = d;
  return VCP_OK;
}
