// The scaled sum chain of the real solver loops on slab-form matrices.  Sine / Cosine (TrigonometrySolversModule.F90:263-411), the
// Paterson-Stockmeyer evaluation (PolynomialSolversModule.F90:165-282), the factorized Chebyshev evaluation
// (ChebyshevSolversModule.F90:250-365) and the inverse-root iteration (RootSolversModule.F90:177-337) all build, with the vocabulary
// at threshold 0,
//   CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A_k, Out, c_k, 0) for k = 1..M; [ScaleMatrix(Out, post)]
// -- up to eight calls that read and rewrite matrices the size of the widest operand.  k_sum_chain<M> reads the runs of Base and
// A_1..A_M once and writes the one output: k_pade_chain's geometry (pade_chain.hip) with one output, M = 1..5 and a trailing
// scaling.
//
// Every merge is AddSparseVectors at threshold 0 as k_sa_axpby (kernels.hip) restates it on runs: the scaled addend is rounded,
// then added; a row both operands hold is kept iff the sum is not zero -- a row that cancels is ABSENT for the next addend; a row one
// operand holds keeps its (non-zero) value.  At threshold 0 no rule looks at the other operand's last row, so ONE sweep decides a
// column.  A scaling by 1.0 leaves the bits as they are, so s == 1 and post == 1 (where the loops make no ScaleMatrix call) need no
// branch.
//
// stat |= 1: a scaled value is exactly zero where an entry is held (compressed columns would store it, no run can); |= 2: runs far
// apart (the hull is not bounded by the inputs' own slots and pads), a slot beyond the output buffer, or an input that is not
// finite -- the pass is refused.
//
// The complex loops' chain (option complex_sum_chain = 2, inside a complex slab session) is the same kernel on double2 elements:
// k_sum_chain<double2, M>, the rules of step_merge (slab_extra.hip) at threshold 0 with real scalars.
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
struct ScRuns {   // one operand in slab form
  const int32_t* first;
  const int32_t* last;
  const int64_t* off;
  const double* val;
};
ScRuns sc_runs(const DevMat& M) { return ScRuns{M.slab->first.p, M.slab->last.p, M.slab->off.p, M.slab->val.p}; }
template <int M>
struct ScIn {   // in[0] = Base, in[1..M] = the addends; s scales Base, c[k] the addend k + 1, post the finished sum
  ScRuns in[M + 1];
  double s, post;
  double c[M];
};

template <typename T>
struct ScCol {   // one column of an operand: p[r] is row r for f <= r <= l (an empty column: f = INT_MAX, l = -1)
  const T* p;
  int f, l;
};
template <typename T>
__device__ inline ScCol<T> sc_col(const ScRuns& R, int j) {
  const int f = R.first[j], l = R.last[j];
  const T* v = reinterpret_cast<const T*>(R.val);
  if (l < f) return ScCol<T>{v, INT_MAX, -1};
  return ScCol<T>{v + (R.off[j] - f), f, l};
}
template <typename T>
__device__ inline T sc_at(const ScCol<T>& c, int r) { return (r >= c.f && r <= c.l) ? c.p[r] : Sc<T>::zero(); }
__device__ inline bool sc_finite(double v) { return isfinite(v); }
__device__ inline bool sc_finite(double2 v) { return isfinite(v.x) && isfinite(v.y); }

// the aligned hull of the runs of all inputs, per column (nothing where all are empty): the slot of the output
template <int M>
__global__ void k_sum_span(ScIn<M> P, int n, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
#pragma unroll
  for (int k = 0; k <= M; ++k)
    if (P.in[k].last[j] >= P.in[k].first[j]) { f = min(f, P.in[k].first[j]); l = max(l, P.in[k].last[j]); }
  span[j] = l >= 0 ? (l / al + 1) * al - f / al * al : 0;
}

// One wave per column, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of Base and the addends, chunks of 64
// rows whose loads (M + 1 operands) are all requested before the first of them is used.  The output goes into the slot at base[j]
// (every row of the hull written: pads and dropped rows zero) with its extent and count.  T = double: the real loops' chain.
// T = double2 (option complex_sum_chain): the same sweep on runs of (re, im) pairs -- slots, spans and `bound` count elements, a
// lane's load and store are 16 bytes --, every scalar real and applied to each part by itself (Sc<double2>::scale), the merge part by
// part (Sc<double2>::add); an entry is held iff it is not (0, 0), so a row that cancels in ONE part stays and only a row that
// cancels in both is absent for the next addend, and only a scaled value that is (0, 0) where an entry is held sets stat bit 1
template <typename T, int M>
__global__ __launch_bounds__(256) void k_sum_chain(int n, ScIn<M> P, int al, const int64_t* __restrict__ base, IsrOut o, int64_t bound,
                                                   unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  ScCol<T> col[M + 1];
  int f = INT_MAX, l = -1, own = 0;   // the hull of the runs, and the rows their own aligned slots hold
#pragma unroll
  for (int k = 0; k <= M; ++k) {
    col[k] = sc_col<T>(P.in[k], j);
    if (col[k].l >= 0) { f = min(f, col[k].f); l = max(l, col[k].l); own += (col[k].l / al + 1) * al - col[k].f / al * al; }
  }
  const int64_t slot = base[j];
  const int a0 = l >= 0 ? f / al * al : 0, a1 = l >= 0 ? (l / al + 1) * al : 0;
  // (runs far apart: their hull is not bounded by the inputs' slots and the pads between them -- refused per column; a column
  // empty in every input is an empty column of the result)
  if (l < 0 || a1 - a0 > own + (M + 1) * al || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
      o.first[j] = INT_MAX; o.last[j] = -1; o.count[j] = 0; o.off[j] = slot;
      if (l >= 0) atomicOr(stat, 2ull);
    }
    return;
  }
  T* __restrict__ d = static_cast<T*>(o.val) + (slot - a0);
  int zk = 0, bad = 0, cnt = 0, kf = INT_MAX, kl = -1;
  for (int r = a0 + lane; r < a1; r += WAVE) {
    T x[M + 1];
#pragma unroll
    for (int k = 0; k <= M; ++k) x[k] = sc_at(col[k], r);
    // CopyMatrix(Base, Out); ScaleMatrix(Out, s)
    bool has = !Sc<T>::is_zero(x[0]);
    T v = has ? Sc<T>::scale(P.s, x[0]) : Sc<T>::zero();
    zk |= (has && Sc<T>::is_zero(v)) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      // IncrementMatrix(A_k, Out, c_k): A = the addend, B = the running value
      const T a = x[k + 1];
      const bool ha = !Sc<T>::is_zero(a);
      const T wa = Sc<T>::scale(P.c[k], a);
      zk |= (ha && Sc<T>::is_zero(wa)) ? 1 : 0;
      if (ha && has) { v = Sc<T>::add(wa, v); has = !Sc<T>::is_zero(v); }
      else if (ha) { v = wa; has = true; }
    }
    // ScaleMatrix(Out, post)
    v = has ? Sc<T>::scale(P.post, v) : Sc<T>::zero();
    zk |= (has && Sc<T>::is_zero(v)) ? 1 : 0;
    d[r] = v;
    cnt += has ? 1 : 0;
    kf = min(kf, has ? r : INT_MAX);
    kl = max(kl, has ? r : -1);
#pragma unroll
    for (int k = 0; k <= M; ++k) bad |= sc_finite(x[k]) ? 0 : 1;
  }
  cnt = (int)wave_sum_i64(cnt);
  kf = wave_min_i32(kf);
  kl = wave_max_i32(kl);
  const bool anyz = __ballot(zk != 0) != 0, anyb = __ballot(bad != 0) != 0;
  if (lane == 0) {
    if (anyz) atomicOr(stat, 1ull);
    if (anyb) atomicOr(stat, 2ull);
    o.first[j] = kf; o.last[j] = kl; o.count[j] = cnt;
    o.off[j] = slot + (cnt ? kf - a0 : 0);
  }
}

// what the pass merges: an unlabelled, zero-free slab form of the chain's kind (all real, or all complex) that is no view (square,
// or a column panel in a panel session)
bool sc_operand(const DevMat& M, bool cplx) {
  return M.expanded() && M.cplx == cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1;
}

template <typename T, int M>
bool sc_run(const DevMat* const* in, double s, const double* coeffs, double post, DevMat& Out) {
  const int n = in[0]->cols, al = std::max(1, in[0]->slab->row_pad);
  ScIn<M> P;
  int64_t slots = 0;
  for (int k = 0; k <= M; ++k) {
    P.in[k] = sc_runs(*in[k]);
    slots += in[k]->slab->slots;
  }
  P.s = s;
  P.post = post;
  for (int k = 0; k < M; ++k) P.c[k] = coeffs[k];
  // (the operands' slots and per column the pads of a hull: what the kernel's per-column rule admits)
  const int64_t bound = slots + 2LL * (M + 1) * al * n;
  FreshSlabs fs(n, 1, bound, Sc<T>::cplx, false);
  fs.why[0] = " a scaled value is exactly zero where an entry is held";   // (complex: both parts)
  fs.why[1] = " runs far apart or an input that is not finite";
  hipLaunchKernelGGL(k_sum_span<M>, dim3(cdiv(n, 256)), dim3(256), 0, stream(), P, n, al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL((k_sum_chain<T, M>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, P, al, fs.base.p, fs.out(0), bound, fs.stat.p);
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
  for (int k = 0; k <= n_addends; ++k) {
    if (!in[k] || !sc_operand(*in[k], Base.cplx) || in[k]->cols != Base.cols || in[k]->rows != Base.rows || in[k]->slab->row_pad != Base.slab->row_pad) return false;
    for (int m = 0; m < k; ++m)
      if (in[m] == in[k]) return false;
  }
  if (Base.cols == 0) return false;
  // (ScaleMatrix by zero and a zero coefficient leave stored zeros, a scalar that is not finite nothing a run can hold)
  if (!std::isfinite(s) || s == 0.0 || !std::isfinite(post) || post == 0.0) return false;
  for (int k = 0; k < n_addends; ++k)
    if (!std::isfinite(coeffs[k]) || coeffs[k] == 0.0) return false;
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
