// regp_host_emulation.cpp -- runs the SOURCE of k_regp_search and k_regs_search (csrc/register.hip, copied into kernels.inc by
// tools/regp_host_emulation.py behind the grid, cell and row-range functions of csrc/epsgrid.hpp) on the host: 256 real threads per workgroup, one workgroup after the other, with
// __syncthreads / __syncthreads_or / __ballot / __shfl built from std::barrier and the atomics from the compiler's
// builtins.  It checks the queue, the barriers and the winner's word of the fused kernel where no GPU is at hand, and can
// be built with -fsanitize=address,undefined.  The base table, the sorted lengths and the target grid are built here the
// way k_regp_bases, the host code and epsgrid.hpp build them.
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>
#include <algorithm>
using std::isfinite; using std::floor; using std::sqrt; using std::fabs;
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, o, sc) __atomic_load_n((p), __ATOMIC_RELAXED)
struct Dim { unsigned x, y, z; };
static thread_local Dim threadIdx, blockIdx;
constexpr int NT = 256;
static std::barrier<> blockbar(NT);
static std::barrier<>* wavebar[4];
static std::atomic<unsigned long long> wmask[4];
static int wval[4][64];
static std::atomic<int> bor;
static void __syncthreads() { blockbar.arrive_and_wait(); }
static int __syncthreads_or(int p) {
  if (p) bor.fetch_or(1);
  blockbar.arrive_and_wait();
  const int r = bor.load();
  blockbar.arrive_and_wait();
  if (threadIdx.x == 0) bor.store(0);
  blockbar.arrive_and_wait();
  return r;
}
static unsigned long long __ballot(int p) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (p) wmask[w].fetch_or(1ull << l);
  wavebar[w]->arrive_and_wait();
  const unsigned long long r = wmask[w].load();
  wavebar[w]->arrive_and_wait();
  if (l == 0) wmask[w].store(0);
  wavebar[w]->arrive_and_wait();
  return r;
}
static int __shfl(int v, int src, int) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  wval[w][l] = v;
  wavebar[w]->arrive_and_wait();
  const int r = wval[w][src];
  wavebar[w]->arrive_and_wait();
  return r;
}
static int __builtin_amdgcn_readfirstlane(int v) { return v; }
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static int __ffsll(long long v) { return __builtin_ffsll(v); }
static uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
  unsigned long long o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return o;
}
namespace mtc {
inline void transform(const double* M, double c0, double c1, double c2, double m[3]) {
  for (int r = 0; r < 3; r++) m[r] = c0 * M[4 * r] + c1 * M[4 * r + 1] + c2 * M[4 * r + 2] + M[4 * r + 3];
}
}
constexpr int RT = 256;
constexpr int RG_QCAP = 2 * RT;
constexpr int RG_MAX_BASES = 4096;
constexpr unsigned long long RG_LOW = (1ull << 33) - 1ull;
#include "kernels.inc"

int main(int argc, char** argv) {
  // input file: int64 ns, nt, nb, step, mirror, sim; double len_tol, inlier, h (cell edge; 0 = one cell), scale_min,
  // scale_max; src, tgt, bases(int32)
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[6]; double pr[5];
  if (fread(hd, 8, 6, f) != 6 || fread(pr, 8, 5, f) != 5) return 2;
  const int64_t ns = hd[0], nt = hd[1], nb = hd[2], step = hd[3]; const int mirror = (int)hd[4]; const bool sim = hd[5] != 0;
  std::vector<double> src(3 * ns), tgt(3 * nt); std::vector<int32_t> bases(2 * nb);
  if (fread(src.data(), 8, 3 * ns, f) != (size_t)(3 * ns) || fread(tgt.data(), 8, 3 * nt, f) != (size_t)(3 * nt) ||
      fread(bases.data(), 4, 2 * nb, f) != (size_t)(2 * nb)) return 2;
  fclose(f);
  for (int w = 0; w < 4; w++) wavebar[w] = new std::barrier<>(64);
  // base table (k_regp_bases's arithmetic through rg_base)
  std::vector<double> tab(6 * nb);
  for (int b = 0; b < nb; b++) { double r[6]; rg_base(&src[3 * bases[2 * b]], &src[3 * bases[2 * b + 1]], r); for (int t = 0; t < 6; t++) tab[(size_t)t * nb + b] = r[t]; }
  std::vector<int32_t> ord;
  for (int b = 0; b < nb; b++) if (tab[b] > 0.0 && tab[b] < INFINITY) ord.push_back(b);
  std::sort(ord.begin(), ord.end(), [&](int x, int y) { return tab[x] < tab[y] || (tab[x] == tab[y] && x < y); });
  std::vector<double> sL; for (int b : ord) sL.push_back(tab[b]);
  // the grid as eg_bin leaves it (finite targets only; h = 0: one cell)
  EpsGrid g{0, 0, 0, 0.0, 1, 1, 1};
  const double h = pr[2];
  if (h > 0) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int i = 0; i < nt; i++) for (int c = 0; c < 3; c++) if (std::isfinite(tgt[3 * i + c])) { lo[c] = std::min(lo[c], tgt[3 * i + c]); hi[c] = std::max(hi[c], tgt[3 * i + c]); }
    g = EpsGrid{lo[0], lo[1], lo[2], 1.0 / h, (int)((hi[0] - lo[0]) / h) + 1, (int)((hi[1] - lo[1]) / h) + 1, (int)((hi[2] - lo[2]) / h) + 1};
  }
  const size_t nc = (size_t)g.Dx * g.Dy * g.Dz;
  std::vector<uint32_t> cellof(nt, 0xFFFFFFFFu), cellstart(nc + 1, 0), cur(nc, 0);
  for (int i = 0; i < nt; i++) {
    const double x = tgt[3 * i], y = tgt[3 * i + 1], z = tgt[3 * i + 2];
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
    const uint32_t c = eg_cell_of(g, x, y, z);
    cellof[i] = c; cellstart[c + 1]++;
  }
  for (size_t c = 0; c < nc; c++) cellstart[c + 1] += cellstart[c];
  std::vector<double> sxyz(3 * nt);
  for (int i = 0; i < nt; i++) if (cellof[i] != 0xFFFFFFFFu) { const uint32_t s = cellstart[cellof[i]] + cur[cellof[i]]++; for (int c = 0; c < 3; c++) sxyz[3 * s + c] = tgt[3 * i + c]; }
  RGScan q{g, cellstart.data(), sxyz.data(), pr[1]};
  std::vector<unsigned long long> key(nb, 0), nhyp(nb, 0);
  RGSearch a{src.data(), step, (int)(ns / step), tgt.data(), (int)nt, RGTab{tab.data(), (int)nb}, sL.data(), ord.data(), (int)ord.size(), pr[0], pr[3], pr[4], mirror ? 2 : 1, q, key.data(), nhyp.data()};
  if (!ord.empty())
    for (unsigned blk = 0; blk < (unsigned)nt; blk++) {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < NT; t++) th.emplace_back([&, t, blk] { threadIdx = Dim{t, 0, 0}; blockIdx = Dim{blk, 0, 0}; if (sim) k_regs_search(a); else k_regp_search(a); });
      for (auto& x : th) x.join();
    }
  FILE* o = fopen(argv[2], "wb");
  fwrite(key.data(), 8, nb, o); fwrite(nhyp.data(), 8, nb, o); fclose(o);
  return 0;
}
