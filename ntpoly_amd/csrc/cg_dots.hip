// Column dot passes for the traces of CGSolver (option cg_dots).  The loop of LinearSolversModule.F90:101-139
// forms R^H R (twice) and P^H Q per iteration only to trace them.  Entry (j, j) of U^H V is the dot product of column j of U with
// column j of V: column-local, no transpose, no SpGEMM.
//
// k_cg_dots<T, FMA, PAIRS>: for every local column j and every pair (U, V) of slab-form operands
//   d_j = the chain over ascending row k of Sc<T>::fmadd(conj(U(k, j)), V(k, j), acc, FMA), acc starting at zero,
//   d_j = Sc<T>::mag(d_j) > threshold ? d_j : 0      (strict, the modulus for complex: the product's pruning rule)
// -- what every product kernel leaves at (j, j) of MatrixMultiply(U^H, V, threshold).  The chain of a column is ONE accumulator
// walked in ascending k by ONE lane (the bits depend on the order: no tree, no wave reduction); rows outside either run add
// nothing; stored zeros inside both runs are multiplied, which changes no bit.
// A slab column is contiguous in memory, so a lane reading its own run would stride by a column's length.  The runs are staged
// through LDS instead: a workgroup takes CG_COLS neighbouring columns and walks the hull of their chains in windows of W rows; its
// four waves read each column's rows of the window with consecutive lanes on consecutive addresses (both members of a pair and
// both pairs in the same sweep), into tiles of pitch W + 1 elements; then lane c of wave p walks column c of pair p through its
// tiles in order.  The pitch is odd in elements: the 32 lanes of a ds_read_b64 group (16 of a ds_read_b128 group) then fall on
// distinct banks for 8-byte and for 16-byte elements alike, and the staging writes of a wave are consecutive.
// The real part of d_j goes into a dense array, one double per local column and pair: no floating-point atomics.
//
// k_cg_trace + k_cg_finish sum that array with the launch shape and the order of k_trace / trace() / finish_sum2 (kernels.hip):
// min(cdiv(cols, 256), 1024) blocks of 256 threads, thread t adds columns t, t + 256 grid, ... in order, the wave butterfly, the four
// waves as (s0 + s1) + (s2 + s3), then the blocks' sums by the fixed tree of k_reduce_sum2.  The running sums start at +0 and a
// kept d_j is not zero, so the +0 of a pruned or absent diagonal entry changes no bit: MatrixTrace of the product, bit for bit.
//
// k_cg_dots_csc: the same chains on packed compressed columns (a merge of the two columns' ascending row lists), one lane per
// column -- for a rank whose panel is not in slab form while the others' are.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "slab_columns.hpp"

namespace ntp {
namespace {

constexpr int CG_COLS = 64;   // columns per workgroup: one lane each in the chain phase
template <typename T>
struct CgWin;                 // rows per window: 128-byte pieces of a column
template <>
struct CgWin<double> { static constexpr int W = 16; };
template <>
struct CgWin<double2> { static constexpr int W = 8; };

struct CgPairs {
  SlabRuns u[2], v[2];
};

template <typename T, bool FMA, int PAIRS>
__global__ __launch_bounds__(256) void k_cg_dots(int n, CgPairs ops, double threshold, double* __restrict__ diag) {
  constexpr int W = CgWin<T>::W, P = W + 1;
  __shared__ T tu[PAIRS][CG_COLS][P], tv[PAIRS][CG_COLS][P];
  __shared__ int sa[PAIRS][CG_COLS], sb[PAIRS][CG_COLS];              // the chain's rows [a, b] per column (empty: a > b)
  __shared__ int sfu[PAIRS][CG_COLS], sfv[PAIRS][CG_COLS];            // first rows of the two runs
  __shared__ long long sou[PAIRS][CG_COLS], sov[PAIRS][CG_COLS];      // their offsets
  const int t = threadIdx.x, c0 = blockIdx.x * CG_COLS;
  if (t < PAIRS * CG_COLS) {
    const int p = t / CG_COLS, c = t % CG_COLS, j = c0 + c;
    int a = 0, b = -1, fu = 0, fv = 0;
    long long ou = 0, ov = 0;
    if (j < n) {
      fu = ops.u[p].first[j];
      fv = ops.v[p].first[j];
      const int lu = ops.u[p].last[j], lv = ops.v[p].last[j];
      if (lu >= fu && lv >= fv) { a = max(fu, fv); b = min(lu, lv); }
      ou = ops.u[p].off[j];
      ov = ops.v[p].off[j];
    }
    sa[p][c] = a; sb[p][c] = b; sfu[p][c] = fu; sfv[p][c] = fv; sou[p][c] = ou; sov[p][c] = ov;
  }
  __syncthreads();
  int lo = INT_MAX, hi = -1;
  for (int p = 0; p < PAIRS; ++p)
    for (int c = 0; c < CG_COLS; ++c)
      if (sb[p][c] >= sa[p][c]) { lo = min(lo, sa[p][c]); hi = max(hi, sb[p][c]); }
  // the chain phase: wave p owns pair p, lane c column c
  const int cp = t / WAVE, cc = t % WAVE;
  const bool walker = cp < PAIRS;
  T acc = Sc<T>::zero();
  int ca = 0, cb = -1;
  if (walker) { ca = sa[cp][cc]; cb = sb[cp][cc]; }
  if (hi >= lo) {   // (uniform: some column of the group has a chain)
    for (int r0 = lo / W * W; r0 <= hi; r0 += W) {
      // every wave stages: element e = (pair, column, row of the window), W consecutive lanes on one column's consecutive rows
      for (int e = t; e < PAIRS * CG_COLS * W; e += 256) {
        const int p = e / (CG_COLS * W), c = (e / W) % CG_COLS, i = e % W, r = r0 + i;
        T xu = Sc<T>::zero(), xv = Sc<T>::zero();
        if (r >= sa[p][c] && r <= sb[p][c]) {   // (inside both runs: the only rows a chain reads)
          xu = reinterpret_cast<const T*>(ops.u[p].val)[sou[p][c] + (r - sfu[p][c])];
          xv = reinterpret_cast<const T*>(ops.v[p].val)[sov[p][c] + (r - sfv[p][c])];
        }
        tu[p][c][i] = xu;
        tv[p][c][i] = xv;
      }
      __syncthreads();
      if (walker) {
        // (every lane at the same i: the reads of a step differ by the column's pitch only)
        const int i0 = ca - r0, i1 = cb - r0;
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (i >= i0 && i <= i1) acc = Sc<T>::fmadd(Sc<T>::conj(tu[cp][cc][i]), tv[cp][cc][i], acc, FMA);
      }
      __syncthreads();
    }
  }
  if (walker && c0 + cc < n) diag[(size_t)cp * n + c0 + cc] = Sc<T>::mag(acc) > threshold ? Sc<T>::re(acc) : 0.0;
}

// one lane per column: the chain over the rows both columns store, in ascending order
template <typename T, bool FMA>
__global__ __launch_bounds__(256) void k_cg_dots_csc(Csc U, Csc V, double threshold, double* __restrict__ diag) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= U.cols) return;
  const T* __restrict__ uv = static_cast<const T*>(U.val);
  const T* __restrict__ vv = static_cast<const T*>(V.val);
  int64_t a = U.outer[j], b = V.outer[j];
  const int64_t ae = U.outer[j + 1], be = V.outer[j + 1];
  T acc = Sc<T>::zero();
  while (a < ae && b < be) {
    const int ra = U.inner[a], rb = V.inner[b];
    if (ra == rb) { acc = Sc<T>::fmadd(Sc<T>::conj(uv[a]), vv[b], acc, FMA); ++a; ++b; }
    else if (ra < rb) ++a;
    else ++b;
  }
  diag[j] = Sc<T>::mag(acc) > threshold ? Sc<T>::re(acc) : 0.0;
}

// k_trace's sum of the dense diagonal of pair blockIdx.y: partial[pair][2 b] = the block's sum, [2 b + 1] = 0
__global__ __launch_bounds__(256) void k_cg_trace(int n, const double* __restrict__ diag, double* __restrict__ partial) {
  __shared__ double sx[4];
  const double* __restrict__ d = diag + (size_t)blockIdx.y * n;
  double x = 0;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) x = __dadd_rn(x, d[j]);
  x = wave_sum_f64(x);
  if (lane_id() == 0) sx[threadIdx.x / WAVE] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* __restrict__ o = partial + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = __dadd_rn(__dadd_rn(sx[0], sx[1]), __dadd_rn(sx[2], sx[3]));
    o[1] = 0.0;
  }
}
// finish_sum2 on the nb <= 1024 block sums of pair blockIdx.x (k_reduce_sum2 with one block): out[pair]
__global__ __launch_bounds__(256) void k_cg_finish(const double* __restrict__ partial, int nb, double* __restrict__ out) {
  __shared__ double sx[256];
  const double* __restrict__ part = partial + 2 * (size_t)blockIdx.x * nb;
  double x = 0;
  for (int i = threadIdx.x; i < nb; i += 256) x = __dadd_rn(x, part[2 * i]);
  sx[threadIdx.x] = x;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sx[threadIdx.x] = __dadd_rn(sx[threadIdx.x], sx[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sx[0];
}

// the sums of `pairs` dense diagonals of n columns each, fetched in one host wait
void cg_trace_sums(const DevBuf<double>& diag, int n, int pairs, double* out) {
  const int nb = std::min(cdiv(n, 256), 1024);
  DevBuf<double> partial((size_t)2 * nb * pairs), res((size_t)pairs);
  hipLaunchKernelGGL(k_cg_trace, dim3(nb, pairs), dim3(256), 0, stream(), n, diag.p, partial.p);
  hipLaunchKernelGGL(k_cg_finish, dim3(pairs), dim3(256), 0, stream(), partial.p, nb, res.p);
  res.download(out, (size_t)pairs);
}

template <typename T, int PAIRS>
void cg_dots_launch(int n, const CgPairs& ops, double threshold, double* diag) {
  const dim3 grid(cdiv(n, CG_COLS)), block(256);
  if (options().spgemm_fma != 0) hipLaunchKernelGGL((k_cg_dots<T, true, PAIRS>), grid, block, 0, stream(), n, ops, threshold, diag);
  else hipLaunchKernelGGL((k_cg_dots<T, false, PAIRS>), grid, block, 0, stream(), n, ops, threshold, diag);
}

// what the pass reads: a slab form in the caller's row order, of one kind and shape; a view's stored zeros are zeros of the run.
// The runs are addressed by first / last / off alone, so slots of any alignment -- and of different alignments -- are read alike
bool cg_operand(const DevMat& M, const DevMat& like) {
  return M.expanded() && !M.slab->labelled() && M.cplx == like.cplx && M.rows == like.rows && M.cols == like.cols;
}

}  // namespace

bool slab_cg_dots(const DevMat& U1, const DevMat& V1, const DevMat* U2, const DevMat* V2, double threshold, double out[2], double* diag_out) {
  if ((U2 == nullptr) != (V2 == nullptr) || !U1.expanded() || !cg_operand(U1, U1) || !cg_operand(V1, U1)) return false;
  if (U2 && (!cg_operand(*U2, U1) || !cg_operand(*V2, U1))) return false;
  const int n = U1.cols, pairs = U2 ? 2 : 1;
  if (n == 0) return false;
  CgPairs ops;
  ops.u[0] = slab_runs(U1);
  ops.v[0] = slab_runs(V1);
  ops.u[1] = slab_runs(U2 ? *U2 : U1);
  ops.v[1] = slab_runs(V2 ? *V2 : V1);
  DevBuf<double> diag((size_t)n * pairs);
  // (statistics, option time_kernels with NTPOLY_AMD_DEBUG_SPGEMM set: the pass between two events, for tools/bench_cg_dots.py)
  const bool timed = options().time_kernels != 0 && std::getenv("NTPOLY_AMD_DEBUG_SPGEMM") != nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (timed) {
    HIP_CHECK(hipEventCreate(&ev[0]));
    HIP_CHECK(hipEventCreate(&ev[1]));
    HIP_CHECK(hipEventRecord(ev[0], stream()));
  }
  if (U1.cplx) {
    if (pairs == 2) cg_dots_launch<double2, 2>(n, ops, threshold, diag.p);
    else cg_dots_launch<double2, 1>(n, ops, threshold, diag.p);
  } else {
    if (pairs == 2) cg_dots_launch<double, 2>(n, ops, threshold, diag.p);
    else cg_dots_launch<double, 1>(n, ops, threshold, diag.p);
  }
  if (timed) HIP_CHECK(hipEventRecord(ev[1], stream()));
  double sums[2] = {0.0, 0.0};
  cg_trace_sums(diag, n, pairs, sums);
  if (timed) {   // (the read-back waited for the stream)
    float ms = 0.f;
    HIP_CHECK(hipEventSynchronize(ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    HIP_CHECK(hipEventDestroy(ev[0]));
    HIP_CHECK(hipEventDestroy(ev[1]));
    // bytes: the slots of every operand of every pair (an upper bound of the rows inside both runs) and the extents
    double slots = (double)U1.slab->slots + (double)V1.slab->slots;
    if (U2) slots += (double)U2->slab->slots + (double)V2->slab->slots;
    std::fprintf(stderr, "[cg dots] timed: n %d pairs %d bytes %.0f ms %.5f\n", n, pairs,
                 8.0 * slots * (U1.cplx ? 2.0 : 1.0) + 32.0 * pairs * (double)n, (double)ms);
  }
  if (diag_out) diag.download(diag_out, (size_t)n);
  out[0] = sums[0];
  if (U2) out[1] = sums[1];
  return true;
}

double cg_dots_columns(const DevMat& U, const DevMat& V, double threshold, double* diag_out) {
  if (U.rows != V.rows || U.cols != V.cols || U.cplx != V.cplx) NTP_FATAL("cg dots: operand mismatch");
  const int n = U.cols;
  if (n == 0 || U.nnz == 0 || V.nnz == 0) {
    if (diag_out) std::fill(diag_out, diag_out + n, 0.0);
    return 0.0;
  }
  DevBuf<double> diag((size_t)n);
  const bool fma = options().spgemm_fma != 0;
  dispatch_type(U.cplx, [&](auto tag) {
    using T = decltype(tag);
    if (fma) hipLaunchKernelGGL((k_cg_dots_csc<T, true>), dim3(cdiv(n, 256)), dim3(256), 0, stream(), view(U), view(V), threshold, diag.p);
    else hipLaunchKernelGGL((k_cg_dots_csc<T, false>), dim3(cdiv(n, 256)), dim3(256), 0, stream(), view(U), view(V), threshold, diag.p);
  });
  double s = 0.0;
  cg_trace_sums(diag, n, 1, &s);
  if (diag_out) diag.download(diag_out, (size_t)n);
  return s;
}

}  // namespace ntp
