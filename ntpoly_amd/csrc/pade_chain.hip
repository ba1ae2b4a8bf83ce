// The two groups of merges of ComputeExponentialPade (ExponentialSolversModule.F90:222-250) on slab-form matrices.  Around its CG
// solve the call builds, with the vocabulary at threshold 0,
//   P1      = 17297280 I + 1995840 B1 + 25200 B2 + 56 B3          TempMat  = 8648640 I + 277200 B1 + 1512 B2 + B3
//   LeftMat = P1 - P2                                              RightMat = P1 + P2
// each as CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k) for k = 1..M -- twelve and four calls that
// read and rewrite matrices the size of the widest power.  Both groups are one chain with two outputs from shared inputs;
// k_pade_chain<M> reads the runs of Base and A_1..A_M once and writes both outputs.
//
// Every merge is AddSparseVectors at threshold 0 as k_sa_axpby (kernels.hip) restates it on runs: the scaled addend is rounded,
// then added; a row both operands hold is kept iff the sum is not zero -- a row that cancels is ABSENT for the next addend; a row one
// operand holds keeps its (non-zero) value.  At threshold 0 no rule looks at the other operand's last row, so ONE sweep decides a
// column.  The two outputs may end with different patterns in the same slots.
//
// stat |= 1: a scaled value is exactly zero where an entry is held (compressed columns would store it, no run can); |= 2: runs far
// apart (the hull is not bounded by the inputs' own slots and pads), a slot beyond the output buffer, or an input that is not
// finite -- the pass is refused.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "device_util.hpp"
#include "fresh_slabs.hpp"
#include "kernels.hpp"

namespace ntp {
namespace {
struct PcRuns {   // one operand in slab form
  const int32_t* first;
  const int32_t* last;
  const int64_t* off;
  const double* val;
};
PcRuns pc_runs(const DevMat& M) { return PcRuns{M.slab->first.p, M.slab->last.p, M.slab->off.p, M.slab->val.p}; }
template <int M>
struct PcIn {   // in[0] = Base, in[1..M] = the addends; s[q] scales Base for output q, c[q][k] the addend k + 1
  PcRuns in[M + 1];
  double s[2];
  double c[2][M];
};

struct PcCol {   // one column of an operand: p[r] is row r for f <= r <= l (an empty column: f = INT_MAX, l = -1)
  const double* p;
  int f, l;
};
__device__ inline PcCol pc_col(const PcRuns& R, int j) {
  const int f = R.first[j], l = R.last[j];
  if (l < f) return PcCol{R.val, INT_MAX, -1};
  return PcCol{R.val + (R.off[j] - f), f, l};
}
__device__ inline double pc_at(const PcCol& c, int r) { return (r >= c.f && r <= c.l) ? c.p[r] : 0.0; }

// the aligned hull of the runs of all inputs, per column (nothing where all are empty): the slot of both outputs
template <int M>
__global__ void k_pade_span(PcIn<M> P, int n, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
#pragma unroll
  for (int k = 0; k <= M; ++k)
    if (P.in[k].last[j] >= P.in[k].first[j]) { f = min(f, P.in[k].first[j]); l = max(l, P.in[k].last[j]); }
  span[j] = l >= 0 ? (l / al + 1) * al - f / al * al : 0;
}

// One wave per column, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of Base and the addends, chunks of 64
// rows whose loads (M + 1 operands) are all requested before the first of them is used.  Output q into the slot at base[j] of
// o[q] (every row of the hull written: pads and dropped rows zero) with its own extent and count.
template <int M>
__global__ __launch_bounds__(256) void k_pade_chain(int n, PcIn<M> P, int al, const int64_t* __restrict__ base, IsrOut o0, IsrOut o1, int64_t bound,
                                                    unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  PcCol col[M + 1];
  int f = INT_MAX, l = -1, own = 0;   // the hull of the runs, and the rows their own aligned slots hold
#pragma unroll
  for (int k = 0; k <= M; ++k) {
    col[k] = pc_col(P.in[k], j);
    if (col[k].l >= 0) { f = min(f, col[k].f); l = max(l, col[k].l); own += (col[k].l / al + 1) * al - col[k].f / al * al; }
  }
  const int64_t slot = base[j];
  const int a0 = l >= 0 ? f / al * al : 0, a1 = l >= 0 ? (l / al + 1) * al : 0;
  // (runs far apart: their hull is not bounded by the inputs' slots and the pads between them -- refused per column; a column
  // empty in every input is an empty column of both results)
  if (l < 0 || a1 - a0 > own + (M + 1) * al || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
      o0.first[j] = INT_MAX; o0.last[j] = -1; o0.count[j] = 0; o0.off[j] = slot;
      o1.first[j] = INT_MAX; o1.last[j] = -1; o1.count[j] = 0; o1.off[j] = slot;
      if (l >= 0) atomicOr(stat, 2ull);
    }
    return;
  }
  double* __restrict__ d0 = static_cast<double*>(o0.val) + (slot - a0);
  double* __restrict__ d1 = static_cast<double*>(o1.val) + (slot - a0);
  int zk = 0, bad = 0;
  int cnt[2] = {0, 0}, kf[2] = {INT_MAX, INT_MAX}, kl[2] = {-1, -1};
  for (int r = a0 + lane; r < a1; r += WAVE) {
    double x[M + 1];
#pragma unroll
    for (int k = 0; k <= M; ++k) x[k] = pc_at(col[k], r);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      // CopyMatrix(Base, Out); ScaleMatrix(Out, s)
      bool has = x[0] != 0.0;
      double v = has ? __dmul_rn(P.s[q], x[0]) : 0.0;
      zk |= (has && v == 0.0) ? 1 : 0;
#pragma unroll
      for (int k = 0; k < M; ++k) {
        // IncrementMatrix(A_k, Out, c_k): A = the addend, B = the running value
        const double a = x[k + 1];
        const bool ha = a != 0.0;
        const double wa = __dmul_rn(P.c[q][k], a);
        if (ha && has) { v = __dadd_rn(wa, v); has = v != 0.0; }
        else if (ha) { v = wa; has = true; zk |= (wa == 0.0) ? 1 : 0; }
      }
      const double o = has ? v : 0.0;
      (q == 0 ? d0 : d1)[r] = o;
      cnt[q] += has ? 1 : 0;
      kf[q] = min(kf[q], has ? r : INT_MAX);
      kl[q] = max(kl[q], has ? r : -1);
    }
#pragma unroll
    for (int k = 0; k <= M; ++k) bad |= isfinite(x[k]) ? 0 : 1;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    cnt[q] = (int)wave_sum_i64(cnt[q]);
    kf[q] = wave_min_i32(kf[q]);
    kl[q] = wave_max_i32(kl[q]);
  }
  const bool anyz = __ballot(zk != 0) != 0, anyb = __ballot(bad != 0) != 0;
  if (lane == 0) {
    if (anyz) atomicOr(stat, 1ull);
    if (anyb) atomicOr(stat, 2ull);
    o0.first[j] = kf[0]; o0.last[j] = kl[0]; o0.count[j] = cnt[0];
    o0.off[j] = slot + (cnt[0] ? kf[0] - a0 : 0);
    o1.first[j] = kf[1]; o1.last[j] = kl[1]; o1.count[j] = cnt[1];
    o1.off[j] = slot + (cnt[1] ? kf[1] - a0 : 0);
  }
}

// what the pass merges: a real, unlabelled, zero-free slab form that is no view (square, or a column panel in a panel session)
bool pc_operand(const DevMat& M) {
  return M.expanded() && !M.cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1;
}

template <int M>
bool pc_run(const DevMat* const* in, const double scales[2], const double* coeffs, DevMat& Out1, DevMat& Out2) {
  const int n = in[0]->cols, al = std::max(1, in[0]->slab->row_pad);
  PcIn<M> P;
  int64_t slots = 0;
  for (int k = 0; k <= M; ++k) {
    P.in[k] = pc_runs(*in[k]);
    slots += in[k]->slab->slots;
  }
  for (int q = 0; q < 2; ++q) {
    P.s[q] = scales[q];
    for (int k = 0; k < M; ++k) P.c[q][k] = coeffs[q * M + k];
  }
  // (the operands' slots and per column the pads of a hull: what the kernel's per-column rule admits)
  const int64_t bound = slots + 2LL * (M + 1) * al * n;
  FreshSlabs fs(n, 2, bound, false, false);
  fs.why[0] = " a scaled value is exactly zero where an entry is held";
  fs.why[1] = " runs far apart or an input that is not finite";
  hipLaunchKernelGGL(k_pade_span<M>, dim3(cdiv(n, 256)), dim3(256), 0, stream(), P, n, al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL(k_pade_chain<M>, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, P, al, fs.base.p, fs.out(0), fs.out(1), bound,
                     fs.stat.p);
  DevMat R[2];
  if (!fs.finish("pade chain", in[0]->rows, al, R)) return false;
  Out1 = std::move(R[0]);
  Out2 = std::move(R[1]);
  return true;
}
}  // namespace

bool slab_pade_chain(const DevMat& Base, const DevMat* const* addends, int n_addends, const double scales[2], const double* coeffs, DevMat& Out1,
                     DevMat& Out2) {
  if (n_addends != 1 && n_addends != 3) return false;
  const DevMat* in[4] = {&Base, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_addends; ++k) in[k + 1] = addends[k];
  for (int k = 0; k <= n_addends; ++k) {
    if (!in[k] || !pc_operand(*in[k]) || in[k]->cols != Base.cols || in[k]->rows != Base.rows || in[k]->slab->row_pad != Base.slab->row_pad) return false;
    for (int m = 0; m < k; ++m)
      if (in[m] == in[k]) return false;
  }
  if (Base.cols == 0) return false;
  // (ScaleMatrix by zero and a zero coefficient leave stored zeros, a scalar that is not finite nothing a run can hold)
  for (int q = 0; q < 2; ++q) {
    if (!std::isfinite(scales[q]) || scales[q] == 0.0) return false;
    for (int k = 0; k < n_addends; ++k)
      if (!std::isfinite(coeffs[q * n_addends + k]) || coeffs[q * n_addends + k] == 0.0) return false;
  }
  return n_addends == 3 ? pc_run<3>(in, scales, coeffs, Out1, Out2) : pc_run<1>(in, scales, coeffs, Out1, Out2);
}

}  // namespace ntp
