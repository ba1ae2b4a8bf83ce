// The two groups of merges of ComputeExponentialPade (ExponentialSolversModule.F90:222-250) on slab-form matrices.  Around its CG
// solve the call builds, with the vocabulary at threshold 0,
//   P1      = 17297280 I + 1995840 B1 + 25200 B2 + 56 B3          TempMat  = 8648640 I + 277200 B1 + 1512 B2 + B3
//   LeftMat = P1 - P2                                              RightMat = P1 + P2
// each as CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k) for k = 1..M -- twelve and four calls that
// read and rewrite matrices the size of the widest power.  Both groups are one chain with two outputs from shared inputs;
// k_pade_chain<M> reads the runs of Base and A_1..A_M once and writes both outputs.
//
// The rules of a merge and of the stat bits, and the sweep itself (hull_sweep), are in slab_columns.hpp.
#include <hip/hip_runtime.h>

#include "slab_columns.hpp"

namespace ntp {
namespace {
// in[0] = Base, in[1..M] = the addends; s[q] scales Base for output q, c[q][k] the addend k + 1.  Stat bit 1: a zero scaled value
// of Base where it is held, and of an addend only where the addend ALONE holds the row -- SumRow (sum_chain.hip) and PolyRow
// (poly_step.hip) flag it wherever the addend is held; a pass that either rule refuses stays refused, so the two are not unified.
template <int M>
struct PadeRow {
  double s[2];
  double c[2][M];
  template <typename Emit>
  __device__ inline void operator()(const double (&x)[M + 1], const Emit& emit, int& zk) const {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      // CopyMatrix(Base, Out); ScaleMatrix(Out, s)
      bool has = x[0] != 0.0;
      double v = has ? Sc<double>::scale(s[q], x[0]) : 0.0;
      zk |= (has && v == 0.0) ? 1 : 0;
#pragma unroll
      for (int k = 0; k < M; ++k) {
        // IncrementMatrix(A_k, Out, c_k): A = the addend, B = the running value
        const bool ha = x[k + 1] != 0.0;
        const double wa = Sc<double>::scale(c[q][k], x[k + 1]);
        merge0(wa, ha, v, has, [&] { zk |= (wa == 0.0) ? 1 : 0; });
      }
      emit(q, has ? v : 0.0, has);
    }
  }
};

template <int M>
__global__ __launch_bounds__(256) void k_pade_chain(int n, SlabIn<M + 1> P, PadeRow<M> row, int al, const int64_t* __restrict__ base, IsrOut o0,
                                                    IsrOut o1, int64_t bound, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const IsrOut out[2] = {o0, o1};
  hull_sweep<double>(j, lane_id(), P, row, al, base, out, bound, stat);
}

template <int M>
bool pc_run(const DevMat* const* in, const double scales[2], const double* coeffs, DevMat& Out1, DevMat& Out2) {
  const int n = in[0]->cols, al = std::max(1, in[0]->slab->row_pad);
  SlabIn<M + 1> P;
  PadeRow<M> row;
  for (int q = 0; q < 2; ++q) {
    row.s[q] = scales[q];
    for (int k = 0; k < M; ++k) row.c[q][k] = coeffs[q * M + k];
  }
  // (the operands' slots and per column the pads of a hull: what the kernel's per-column rule admits)
  const int64_t bound = slab_in(in, P) + 2LL * (M + 1) * al * n;
  FreshSlabs fs(n, 2, bound, false, false);
  fs.why[0] = SLAB_WHY_ZERO;
  fs.why[1] = SLAB_WHY_APART;
  hull_slots(P, n, al, fs);
  hipLaunchKernelGGL(k_pade_chain<M>, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, P, row, al, fs.base.p, fs.out(0), fs.out(1),
                     bound, fs.stat.p);
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
  for (int k = 0; k <= n_addends; ++k)
    if (!in[k] || !slab_merge_operand(*in[k], false)) return false;
  if (!same_frame(in, n_addends + 1, true) || Base.cols == 0) return false;
  for (int q = 0; q < 2; ++q) {
    if (!scalar_usable(scales[q])) return false;
    for (int k = 0; k < n_addends; ++k)
      if (!scalar_usable(coeffs[q * n_addends + k])) return false;
  }
  return n_addends == 3 ? pc_run<3>(in, scales, coeffs, Out1, Out2) : pc_run<1>(in, scales, coeffs, Out1, Out2);
}

}  // namespace ntp
