// The scaled sum chain of the real solver loops on slab-form matrices.  Sine / Cosine (TrigonometrySolversModule.F90:263-411), the
// Paterson-Stockmeyer evaluation (PolynomialSolversModule.F90:165-282), the factorized Chebyshev evaluation
// (ChebyshevSolversModule.F90:250-365) and the inverse-root iteration (RootSolversModule.F90:177-337) all build, with the vocabulary
// at threshold 0,
//   CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k, 0) for k = 1..M; [ScaleMatrix(Out, post)]
// -- up to eight calls that read and rewrite matrices the size of the widest operand.  k_sum_chain<M> reads the runs of Base and
// A_1..A_M once and writes the one output: k_pade_chain's geometry (pade_chain.hip) with one output, M = 1..5 and a trailing
// scaling.
//
// The rules of a merge and of the stat bits, and the sweep itself (hull_sweep), are in slab_columns.hpp.  A scaling by 1.0 leaves the
// bits as they are, so s == 1 and post == 1 (where the loops make no ScaleMatrix call) need no branch.
//
// The complex loops' chain (option complex_sum_chain = 2, inside a complex slab session) is the same kernel on double2 elements:
// k_sum_chain<double2, M>, the rules of step_merge (slab_extra.hip) at threshold 0 with real scalars.
#include <hip/hip_runtime.h>

#include "slab_columns.hpp"

namespace ntp {
namespace {
// in[0] = Base, in[1..M] = the addends; s scales Base, c[k] the addend k + 1, post the finished sum.  Stat bit 1: a zero scaled
// value WHEREVER the addend is held, and a zero of the trailing scaling -- PadeRow (pade_chain.hip) flags it only where the addend
// alone holds the row; a pass that either rule refuses stays refused, so the two are not unified.
// T = double2 (option complex_sum_chain): runs of (re, im) pairs -- slots, spans and `bound` count elements, a lane's load and
// store are 16 bytes --, every scalar real and applied to each part by itself (Sc<double2>::scale), the merge part by part
// (Sc<double2>::add); an entry is held iff it is not (0, 0), so a row that cancels in ONE part stays and only a row that cancels in
// both is absent for the next addend, and only a scaled value that is (0, 0) where an entry is held sets stat bit 1
template <typename T, int M>
struct SumRow {
  double s, post;
  double c[M];
  template <typename Emit>
  __device__ inline void operator()(const T (&x)[M + 1], const Emit& emit, int& zk) const {
    // CopyMatrix(Base, Out); ScaleMatrix(Out, s)
    bool has = !Sc<T>::is_zero(x[0]);
    T v = has ? Sc<T>::scale(s, x[0]) : Sc<T>::zero();
    zk |= (has && Sc<T>::is_zero(v)) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      // IncrementMatrix(A_k, Out, c_k): A = the addend, B = the running value
      const bool ha = !Sc<T>::is_zero(x[k + 1]);
      const T wa = Sc<T>::scale(c[k], x[k + 1]);
      zk |= (ha && Sc<T>::is_zero(wa)) ? 1 : 0;
      merge0(wa, ha, v, has);
    }
    // ScaleMatrix(Out, post)
    v = has ? Sc<T>::scale(post, v) : Sc<T>::zero();
    zk |= (has && Sc<T>::is_zero(v)) ? 1 : 0;
    emit(0, v, has);
  }
};

template <typename T, int M>
__global__ __launch_bounds__(256) void k_sum_chain(int n, SlabIn<M + 1> P, SumRow<T, M> row, int al, const int64_t* __restrict__ base, IsrOut o,
                                                   int64_t bound, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const IsrOut out[1] = {o};
  hull_sweep<T>(j, lane_id(), P, row, al, base, out, bound, stat);
}

template <typename T, int M>
bool sc_run(const DevMat* const* in, double s, const double* coeffs, double post, DevMat& Out) {
  const int n = in[0]->cols, al = std::max(1, in[0]->slab->row_pad);
  SlabIn<M + 1> P;
  SumRow<T, M> row;
  row.s = s;
  row.post = post;
  for (int k = 0; k < M; ++k) row.c[k] = coeffs[k];
  // (the operands' slots and per column the pads of a hull: what the kernel's per-column rule admits)
  const int64_t bound = slab_in(in, P) + 2LL * (M + 1) * al * n;
  FreshSlabs fs(n, 1, bound, Sc<T>::cplx, false);
  fs.why[0] = SLAB_WHY_ZERO;
  fs.why[1] = SLAB_WHY_APART;
  hull_slots(P, n, al, fs);
  hipLaunchKernelGGL((k_sum_chain<T, M>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, P, row, al, fs.base.p, fs.out(0), bound,
                     fs.stat.p);
  DevMat R[1];
  if (!fs.finish(Sc<T>::cplx ? "complex sum chain" : "sum chain", in[0]->rows, al, R)) return false;
  Out = std::move(R[0]);
  return true;
}
}  // namespace

bool slab_sum_chain(const DevMat& Base, double s, const DevMat* const* addends, const double* coeffs, int n_addends, double post, DevMat& Out) {
  if (n_addends < 1 || n_addends > 5) return false;
  const DevMat* in[6] = {&Base, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_addends; ++k) in[k + 1] = addends[k];
  for (int k = 0; k <= n_addends; ++k)
    if (!in[k] || !slab_merge_operand(*in[k], Base.cplx)) return false;
  if (!same_frame(in, n_addends + 1, true) || Base.cols == 0) return false;
  if (!scalar_usable(s) || !scalar_usable(post)) return false;
  for (int k = 0; k < n_addends; ++k)
    if (!scalar_usable(coeffs[k])) return false;
  bool done = false;
  dispatch_type(Base.cplx, [&](auto tag) {
    using T = decltype(tag);
    switch (n_addends) {
      case 1: done = sc_run<T, 1>(in, s, coeffs, post, Out); break;
      case 2: done = sc_run<T, 2>(in, s, coeffs, post, Out); break;
      case 3: done = sc_run<T, 3>(in, s, coeffs, post, Out); break;
      case 4: done = sc_run<T, 4>(in, s, coeffs, post, Out); break;
      default: done = sc_run<T, 5>(in, s, coeffs, post, Out); break;
    }
  });
  return done;
}

}  // namespace ntp
