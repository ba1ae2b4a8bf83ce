// Small companions of the slab algebra (kernels.hip, last section).
// (1) Statistics that are only computed when the kernel timers are on: the intermediate products of C = A B for
//     operands in slab form -- sum over the entries B(k, j) of the entries of A(:, k) -- which the compressed-column
//     paths get from their plans (products per second).
// (2) IncrementMatrix(Identity, B, alpha) with threshold 0 on a slab-form B whose diagonal lies inside its runs: one
//     value per column changes, in place, instead of a merge pass over the whole matrix (AddSparseVectors rules for the
//     one row both columns can share: both present -> alpha + b kept unless exactly zero; B has a hole there -> alpha).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "device_util.hpp"
#include "fresh_slabs.hpp"
#include "slab_columns.hpp"
#include "kernels.hpp"

namespace ntp {
namespace {
__global__ __launch_bounds__(256) void k_sa_products(int n, const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                     const int64_t* __restrict__ off, const double* __restrict__ val,
                                                     const int32_t* __restrict__ acount, int acols, unsigned long long* __restrict__ out) {
  __shared__ long long red[4];
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  long long p = 0;
  if (j < n) {
    const int f = first[j], l = last[j];
    if (l >= f) {
      const double* __restrict__ v = val + (off[j] - f);
      for (int k = f + lane_id(); k <= l; k += WAVE)
        if (v[k] != 0.0 && k < acols) p += acount[k];
    }
  }
  p = wave_sum_i64(p);
  if (lane_id() == 0) red[threadIdx.x / WAVE] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long t = red[0] + red[1] + red[2] + red[3];
    if (t) atomicAdd(out, (unsigned long long)t);
  }
}
}  // namespace

namespace {
// pass 1 (apply = 0): what would happen, without touching anything -- st[0] |= 1: a diagonal outside its column's run
// (the run would have to grow), |= 2: a diagonal that cancels at the end of its run (the run would have to shrink);
// st[1] += change of the entry count.  pass 2 (apply = 1): the values and the per-column counts.
__global__ __launch_bounds__(256) void k_sa_add_diagonal(int n, const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                         const int64_t* __restrict__ off, double* __restrict__ val,
                                                         int32_t* __restrict__ count, int col_offset, double alpha, int apply,
                                                         unsigned long long* __restrict__ st) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  int flag = 0, delta = 0;
  if (j < n) {
    const int d = j + col_offset, f = first[j], l = last[j];
    if (l < f || d < f || d > l) {
      flag = 1;
    } else {
      double* p = val + (off[j] + (d - f));
      const double old = *p;
      const bool hb = old != 0.0;
      const double s = hb ? __dadd_rn(alpha, old) : alpha;
      const bool keep = fabs(s) > 0.0;
      if (!keep && (d == f || d == l)) flag = 2;
      delta = (keep ? 1 : 0) - (hb ? 1 : 0);
      if (apply) {
        *p = keep ? s : 0.0;
        count[j] += delta;
      }
    }
  }
  if (!apply) {
    const unsigned long long any = __ballot(flag != 0);
    if (any) {
      int fl = flag;
      for (int o = 32; o > 0; o >>= 1) fl |= __shfl_xor(fl, o, WAVE);
      if (lane_id() == 0) atomicOr(st, (unsigned long long)fl);
    }
    const long long dsum = wave_sum_i64(delta);
    if (lane_id() == 0 && dsum) atomicAdd(st + 1, (unsigned long long)dsum);
  }
}
}  // namespace

// B <- B + alpha I (IncrementMatrix(Identity, B, alpha, 0)); false: not done (B untouched) -- the caller merges
bool slab_add_diagonal(DevMat& B, double alpha, int32_t col_offset) {
  if (!B.expanded() || B.cplx || (B.rows != B.cols && !slab_panels_ok()) || B.slab->labelled() || B.slab->origin || B.zero_free != 1 || alpha == 0.0) return false;
  SlabForm& f = *B.slab;
  const int n = B.cols;
  DevBuf<unsigned long long> st(2);
  st.zero();
  hipLaunchKernelGGL(k_sa_add_diagonal, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, f.first.p, f.last.p, f.off.p, f.val.p, f.count.p,
                     col_offset, alpha, 0, st.p);
  unsigned long long h[2] = {0, 0};
  {
    ScalarFetch ft;
    ft.add(st.p, 2, h);
    ft.run();
  }
  if (h[0] != 0) return false;
  hipLaunchKernelGGL(k_sa_add_diagonal, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, f.first.p, f.last.p, f.off.p, f.val.p, f.count.p,
                     col_offset, alpha, 1, st.p);
  B.nnz += (long long)h[1];
  f.tiles.release();      // (the multiplier tiles held the old diagonal; the next step's plan depends on the extents only)
  f.tile_off.release();
  f.amax.release();       // (SlabForm::amax: the diagonal changed in place)
  return true;
}

// ------------------------------------------------------------------ TRS4's polynomial chain in two passes
// DensityMatrixSolversModule.F90:590-627 builds, with IncrementMatrix at threshold 0,
//   Fx = 4 X - 3 X2,   Gx = (I - 2 X) + X2,   trace_fx = dot(X2, Fx),   trace_gx = dot(X2, Gx),   P = Fx + sigma Gx
// element by element: fx = 4 x + (-3 x2), gx = x2 + ((-2 x) + d) (d = 1 on the diagonal), p = fx + sigma gx, every
// operation rounded on its own and an absent entry entering as zero (adding an exact zero changes nothing, so the values
// are those of the sequence of merges; an entry of the result is where the value is not zero).  Pass 1 reads X and X2
// and leaves the two dots; pass 2 reads them again and writes P -- instead of four merges and two dots over
// materialised Fx and Gx.
// On complex operands (option complex_trs4) every scalar of the chain (4, -3, -2, 1, sigma) is still real, and a real scalar
// times a complex value is a componentwise product: each part of an entry goes through the real trs4_elem on its own, the
// identity adding (1, 0) on the diagonal row.  The traces are the real parts of DotMatrix = sum conj(x2) fx and sum conj(x2) gx,
// x2.re f.re + x2.im f.im with each product and each sum rounded (the terms of k_sa_dot_trace_c); an entry of P exists where
// either part is not zero (the complex merges keep an entry by its modulus at threshold 0).  Runs of double2: 16 bytes per
// lane, consecutive lanes on consecutive rows.  No LDS, no scratch, either kind.
namespace {
template <typename T>
struct Trs4Elem {
  T fx, gx;
};
__device__ inline Trs4Elem<double> trs4_elem(double x, double x2, double d) {
  Trs4Elem<double> e;
  e.fx = __dadd_rn(__dmul_rn(4.0, x), __dmul_rn(-3.0, x2));
  e.gx = __dadd_rn(x2, __dadd_rn(__dmul_rn(-2.0, x), d));
  return e;
}
__device__ inline Trs4Elem<double2> trs4_elem(double2 x, double2 x2, double d) {
  const Trs4Elem<double> re = trs4_elem(x.x, x2.x, d), im = trs4_elem(x.y, x2.y, 0.0);
  Trs4Elem<double2> e;
  e.fx = make_double2(re.fx, im.fx);
  e.gx = make_double2(re.gx, im.gx);
  return e;
}
// one term of dot(X2, F): the real part of conj(x2) f
__device__ inline double trs4_dot(double x2, double f) { return __dmul_rn(x2, f); }
__device__ inline double trs4_dot(double2 x2, double2 f) { return __dadd_rn(__dmul_rn(x2.x, f.x), __dmul_rn(x2.y, f.y)); }
// fx + sigma gx (complex: each part on its own, the product and the sum of one part before the other's)
__device__ inline double trs4_p(double fx, double sigma, double gx) { return __dadd_rn(fx, __dmul_rn(sigma, gx)); }
__device__ inline double2 trs4_p(double2 fx, double sigma, double2 gx) { return make_double2(trs4_p(fx.x, sigma, gx.x), trs4_p(fx.y, sigma, gx.y)); }
// what is stored for p: p where it is an entry, zero elsewhere (the pair rebuilt, not selected: the code of both kinds stays what it was)
__device__ inline double trs4_stored(bool keep, double p, double zero) { return keep ? p : zero; }
__device__ inline double2 trs4_stored(bool keep, double2 p, double2 zero) { return keep ? make_double2(p.x, p.y) : zero; }
// T = double, or double2 on runs of (re, im) pairs: base, bound and the slots of `out` count entries of T.
// MODE 0: part[2 j] = sum x2 fx, part[2 j + 1] = sum x2 gx of column j (summed by k_sa_sum_pairs).  MODE 1: out = fx + sigma gx into the slot at
// base[j] (aligned union of the runs and the diagonal), kept count / first / last per column.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_sa_trs4(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                 const int64_t* __restrict__ offa, const T* __restrict__ va,
                                                 const int32_t* __restrict__ fb, const int32_t* __restrict__ lb,
                                                 const int64_t* __restrict__ offb, const T* __restrict__ vb, int col_offset,
                                                 double sigma, int al, const int64_t* __restrict__ base, double* __restrict__ part,
                                                 T* __restrict__ out, int32_t* __restrict__ ofirst, int32_t* __restrict__ olast,
                                                 int32_t* __restrict__ ocount, int64_t* __restrict__ ooff, int64_t bound,
                                                 unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = fa[j], lA = la[j], fB = fb[j], lB = lb[j], dg = j + col_offset;
  const bool anyA = lA >= fA, anyB = lB >= fB;
  int f = dg, l = dg;   // (the identity's entry is always there)
  if (anyA) { f = min(f, fA); l = max(l, lA); }
  if (anyB) { f = min(f, fB); l = max(l, lB); }
  const int a0 = f / al * al, a1 = (l / al + 1) * al;
  const T* __restrict__ pa = anyA ? va + (offa[j] - fA) : va;
  const T* __restrict__ pb = anyB ? vb + (offb[j] - fB) : vb;
  const T zero = Sc<T>::zero();
  if (MODE == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int r = a0 + lane; r < a1; r += WAVE) {
      const T x = (anyA && r >= fA && r <= lA) ? pa[r] : zero;
      const T x2 = (anyB && r >= fB && r <= lB) ? pb[r] : zero;
      const Trs4Elem<T> e = trs4_elem(x, x2, r == dg ? 1.0 : 0.0);
      s0 = __dadd_rn(s0, trs4_dot(x2, e.fx));
      s1 = __dadd_rn(s1, trs4_dot(x2, e.gx));
    }
    s0 = wave_sum_f64(s0);
    s1 = wave_sum_f64(s1);
    if (lane == 0) { part[2 * (size_t)j] = s0; part[2 * (size_t)j + 1] = s1; }
  } else {
    const int64_t slot = base[j];
    if (slot + (int64_t)(a1 - a0) > bound) {   // (runs far apart: the union extent does not fit the output -- refused by the host)
      if (lane == 0) { ofirst[j] = INT_MAX; olast[j] = -1; ocount[j] = 0; ooff[j] = slot; atomicOr(stat, 2ull); }
      return;
    }
    T* __restrict__ dst = out + (slot - a0);
    int cnt = 0, kf = INT_MAX, kl = -1;
    for (int r = a0 + lane; r < a1; r += WAVE) {
      const T x = (anyA && r >= fA && r <= lA) ? pa[r] : zero;
      const T x2 = (anyB && r >= fB && r <= lB) ? pb[r] : zero;
      const Trs4Elem<T> e = trs4_elem(x, x2, r == dg ? 1.0 : 0.0);
      const T p = trs4_p(e.fx, sigma, e.gx);
      const bool keep = !Sc<T>::is_zero(p);   // (complex: where either part is not zero)
      dst[r] = trs4_stored(keep, p, zero);
      cnt += keep ? 1 : 0;
      kf = min(kf, keep ? r : INT_MAX);
      kl = max(kl, keep ? r : -1);
    }
    cnt = (int)wave_sum_i64(cnt);
    kf = wave_min_i32(kf);
    kl = wave_max_i32(kl);
    if (lane == 0) {
      ofirst[j] = kf; olast[j] = kl; ocount[j] = cnt;
      ooff[j] = slot + (cnt ? kf - a0 : 0);
    }
  }
}
__global__ void k_sa_trs4_span(const int32_t* __restrict__ fa, const int32_t* __restrict__ la, const int32_t* __restrict__ fb,
                               const int32_t* __restrict__ lb, int n, int col_offset, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = j + col_offset, l = j + col_offset;
  if (la[j] >= fa[j]) { f = min(f, fa[j]); l = max(l, la[j]); }
  if (lb[j] >= fb[j]) { f = min(f, fb[j]); l = max(l, lb[j]); }
  span[j] = (l / al + 1) * al - f / al * al;
}
// the tail of a traces-style pass: the n pairs of `part` summed member by member, both sums fetched in the pass's one host wait
void fetch_pair_sums(const DevBuf<double>& part, int n, double out2[2]) {
  DevBuf<double> res(2);
  sum_pairs_async(part.p, n, res.p);
  ScalarFetch ft;
  ft.add(res.p, 2, out2);
  ft.run();
}
bool trs4_operands(const DevMat& X, const DevMat& X2) {
  auto ok = [](const DevMat& M) {
    return M.expanded() && !M.cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1;
  };
  return ok(X) && ok(X2) && X.cols == X2.cols && X.slab->row_pad == X2.slab->row_pad;
}
template <typename T>
bool trs4_traces_run(const DevMat& X, const DevMat& X2, int32_t col_offset, double* trace_fx, double* trace_gx) {
  const SlabForm &fa = *X.slab, &fb = *X2.slab;
  const int n = X.cols;
  DevBuf<double> part((size_t)2 * n);
  hipLaunchKernelGGL((k_sa_trs4<T, 0>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p,
                     reinterpret_cast<const T*>(fa.val.p), fb.first.p, fb.last.p, fb.off.p, reinterpret_cast<const T*>(fb.val.p), col_offset, 0.0,
                     std::max(1, fa.row_pad), (const int64_t*)nullptr, part.p, (T*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (unsigned long long*)nullptr);
  double d[2] = {0.0, 0.0};
  fetch_pair_sums(part, n, d);
  *trace_fx = d[0];
  *trace_gx = d[1];
  return true;
}
// P as a fresh slab-form matrix; false: a union extent beyond the output buffer (runs far apart) -- the caller takes the vocabulary calls
template <typename T>
bool trs4_operand_run(const DevMat& X, const DevMat& X2, double sigma, int32_t col_offset, DevMat& Out) {
  const SlabForm &fa = *X.slab, &fb = *X2.slab;
  const int n = X.cols, al = std::max(1, fa.row_pad);
  const int64_t bound = fa.slots + fb.slots + 4LL * al * n;   // (slots of T)
  FreshSlabs fs(n, 1, bound, Sc<T>::cplx, false);
  hipLaunchKernelGGL(k_sa_trs4_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), fa.first.p, fa.last.p, fb.first.p, fb.last.p, n, col_offset,
                     al, fs.span.p);
  fs.scan();
  const IsrOut o = fs.out(0);
  hipLaunchKernelGGL((k_sa_trs4<T, 1>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p,
                     reinterpret_cast<const T*>(fa.val.p), fb.first.p, fb.last.p, fb.off.p, reinterpret_cast<const T*>(fb.val.p), col_offset, sigma,
                     al, fs.base.p, (double*)nullptr, static_cast<T*>(o.val), o.first, o.last, o.count, o.off, bound, fs.stat.p);
  DevMat R;
  if (!fs.finish("trs4 operand", X.rows, al, &R)) return false;
  Out = std::move(R);
  return true;
}
}  // namespace

bool trs4_operands_c(const DevMat& X, const DevMat& X2) {
  auto ok = [](const DevMat& M) { return sa_operand_c(M) && M.zero_free == 1; };   // (no labelled form, no read-only view)
  return ok(X) && ok(X2) && X.cols == X2.cols && X.rows == X2.rows && X.slab->row_pad == X2.slab->row_pad;
}

bool slab_trs4_traces(const DevMat& X, const DevMat& X2, int32_t col_offset, double* trace_fx, double* trace_gx) {
  return trs4_operands(X, X2) && trs4_traces_run<double>(X, X2, col_offset, trace_fx, trace_gx);
}
bool slab_trs4_traces_c(const DevMat& X, const DevMat& X2, int32_t col_offset, double* trace_fx, double* trace_gx) {
  return trs4_operands_c(X, X2) && trs4_traces_run<double2>(X, X2, col_offset, trace_fx, trace_gx);
}
bool slab_trs4_operand(const DevMat& X, const DevMat& X2, double sigma, int32_t col_offset, DevMat& Out) {
  return trs4_operands(X, X2) && trs4_operand_run<double>(X, X2, sigma, col_offset, Out);
}
bool slab_trs4_operand_c(const DevMat& X, const DevMat& X2, double sigma, int32_t col_offset, DevMat& Out) {
  return trs4_operands_c(X, X2) && trs4_operand_run<double2>(X, X2, sigma, col_offset, Out);
}

// ------------------------------------------------------------------ MatrixNorm(alpha A + beta B) without the sum
// The loops of SignFunction, Invert and the square roots build a difference (Out - Temp2, I - Temp1, I - X) only to
// take its norm (max column abs-sum) for the convergence test.  One pass over the two runs of every column: the
// element is (alpha a) + (beta b) as the merge would compute it, an entry the merge drops (an exact zero) adds nothing.
namespace {
__global__ __launch_bounds__(256) void k_sa_norm_axpby(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                       const int64_t* __restrict__ offa, const double* __restrict__ va,
                                                       const int32_t* __restrict__ fb, const int32_t* __restrict__ lb,
                                                       const int64_t* __restrict__ offb, const double* __restrict__ vb, double alpha,
                                                       double beta, double* __restrict__ colsum) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = fa[j], lA = la[j], fB = fb[j], lB = lb[j];
  const bool anyA = lA >= fA, anyB = lB >= fB;
  double s = 0.0;
  if (anyA || anyB) {
    const int f = anyA ? (anyB ? min(fA, fB) : fA) : fB, l = anyA ? (anyB ? max(lA, lB) : lA) : lB;
    const double* __restrict__ pa = anyA ? va + (offa[j] - fA) : va;
    const double* __restrict__ pb = anyB ? vb + (offb[j] - fB) : vb;
    for (int r = f + lane; r <= l; r += WAVE) {
      const double a = (anyA && r >= fA && r <= lA) ? pa[r] : 0.0;
      const double b = (anyB && r >= fB && r <= lB) ? pb[r] : 0.0;
      s = __dadd_rn(s, fabs(__dadd_rn(__dmul_rn(alpha, a), __dmul_rn(beta, b))));
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) colsum[j] = s;
}
}  // namespace

bool slab_norm_axpby(const DevMat& A, const DevMat& B, double alpha, double beta, double* out) {
  auto ok = [](const DevMat& M) { return M.expanded() && !M.cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled(); };
  if (!ok(A) || !ok(B) || A.cols != B.cols) return false;
  const SlabForm &fa = *A.slab, &fb = *B.slab;
  const int n = A.cols;
  DevBuf<double> cs((size_t)n);
  hipLaunchKernelGGL(k_sa_norm_axpby, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p, fa.val.p,
                     fb.first.p, fb.last.p, fb.off.p, fb.val.p, alpha, beta, cs.p);
  *out = max_of(cs, (size_t)n);
  return true;
}

// ------------------------------------------------------------------ complex operands in slab form (kernels.hpp slab_enter_c)
namespace {
// column j: the diagonal entry (global row col_offset + j) must be stored; newval[j] = alpha + it (AddSparseVectors: alpha * 1
// rounded, then added); flag bit 0: no diagonal entry, bit 1: the sum is zero (the merge would drop it)
__global__ void k_sa_diag_c(int n, const int32_t* __restrict__ first, const int32_t* __restrict__ last, const int64_t* __restrict__ off,
                            double2* __restrict__ val, int col_offset, double alpha, int apply, double2* __restrict__ newval, int* __restrict__ flag) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int d = j + col_offset, f = first[j], l = last[j];
  if (apply) {
    val[off[j] + (d - f)] = newval[j];
    return;
  }
  int fl = 0;
  if (l < f || d < f || d > l) {
    fl = 1;
  } else {
    const double2 old = val[off[j] + (d - f)];
    if (old.x == 0.0 && old.y == 0.0) {
      fl = 1;
    } else {
      const double2 one = make_double2(1.0, 0.0);
      const double2 nv = Sc<double2>::add(Sc<double2>::scale(alpha, one), old);
      newval[j] = nv;
      if (nv.x == 0.0 && nv.y == 0.0) fl = 2;
    }
  }
  if (fl) atomicOr(flag, fl);
}
__global__ __launch_bounds__(256) void k_sa_norm_axpby_c(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                         const int64_t* __restrict__ offa, const double2* __restrict__ va,
                                                         const int32_t* __restrict__ fb, const int32_t* __restrict__ lb,
                                                         const int64_t* __restrict__ offb, const double2* __restrict__ vb, double alpha,
                                                         double beta, double* __restrict__ colsum) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = fa[j], lA = la[j], fB = fb[j], lB = lb[j];
  const bool anyA = lA >= fA, anyB = lB >= fB;
  double s = 0.0;
  if (anyA || anyB) {
    const int f = anyA ? (anyB ? min(fA, fB) : fA) : fB, l = anyA ? (anyB ? max(lA, lB) : lA) : lB;
    const double2* __restrict__ pa = anyA ? va + (offa[j] - fA) : va;
    const double2* __restrict__ pb = anyB ? vb + (offb[j] - fB) : vb;
    for (int r = f + lane; r <= l; r += WAVE) {
      const double2 a = (anyA && r >= fA && r <= lA) ? pa[r] : make_double2(0.0, 0.0);
      const double2 b = (anyB && r >= fB && r <= lB) ? pb[r] : make_double2(0.0, 0.0);
      const double2 v = Sc<double2>::add(Sc<double2>::scale(alpha, a), Sc<double2>::scale(beta, b));
      s = __dadd_rn(s, Sc<double2>::mag(v));
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) colsum[j] = s;
}
}  // namespace

// B <- B + alpha I on a complex slab-form matrix, in place; false: a column without a stored diagonal entry or a zero sum
// (B untouched: the caller packs and merges)
bool slab_add_diagonal_c(DevMat& B, double alpha, int32_t col_offset) {
  if (!sa_operand_c(B) || B.zero_free != 1 || alpha == 0.0) return false;
  SlabForm& f = *B.slab;
  const int n = B.cols;
  DevBuf<double> newval((size_t)2 * n);
  DevBuf<int> flag(2);
  flag.zero();
  hipLaunchKernelGGL(k_sa_diag_c, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, f.first.p, f.last.p, f.off.p, reinterpret_cast<double2*>(f.val.p),
                     col_offset, alpha, 0, reinterpret_cast<double2*>(newval.p), flag.p);
  long long h = 0;
  {
    ScalarFetch ft;
    ft.add(flag.p, 1, &h);
    ft.run();
  }
  if ((int)(h & 0xffffffffll) != 0) return false;
  hipLaunchKernelGGL(k_sa_diag_c, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, f.first.p, f.last.p, f.off.p, reinterpret_cast<double2*>(f.val.p),
                     col_offset, alpha, 1, reinterpret_cast<double2*>(newval.p), flag.p);
  return true;
}

// MatrixNorm(alpha A + beta B) of two complex slab-form matrices, nothing built
bool slab_norm_axpby_c(const DevMat& A, const DevMat& B, double alpha, double beta, double* out) {
  if (!sa_readable_c(A) || !sa_readable_c(B) || A.cols != B.cols) return false;   // (a view's stored zero adds nothing to a column sum)
  const SlabForm &fa = *A.slab, &fb = *B.slab;
  const int n = A.cols;
  DevBuf<double> cs((size_t)n);
  hipLaunchKernelGGL(k_sa_norm_axpby_c, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p,
                     reinterpret_cast<const double2*>(fa.val.p), fb.first.p, fb.last.p, fb.off.p, reinterpret_cast<const double2*>(fb.val.p), alpha,
                     beta, cs.p);
  *out = max_of(cs, (size_t)n);
  return true;
}

// ------------------------------------------------------------------ MatrixTrace of a slab-form matrix
namespace {
__global__ __launch_bounds__(256) void k_sa_diag(int n, const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                 const int64_t* __restrict__ off, const double* __restrict__ val, int col_offset,
                                                 double* __restrict__ part) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int d = j + col_offset, f = first[j], l = last[j];
  part[2 * (size_t)j] = (l >= f && d >= f && d <= l) ? val[off[j] + (d - f)] : 0.0;
  part[2 * (size_t)j + 1] = 0.0;
}
}  // namespace

bool slab_trace(const DevMat& A, int32_t col_offset, double* out) {
  if (!A.expanded() || A.cplx || A.slab->labelled()) return false;
  const SlabForm& f = *A.slab;
  const int n = A.cols;
  DevBuf<double> part((size_t)2 * n), res(2);
  hipLaunchKernelGGL(k_sa_diag, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, f.first.p, f.last.p, f.off.p, f.val.p, col_offset, part.p);
  sum_pairs_async(part.p, n, res.p);
  unsigned long long h[2] = {0, 0};
  ScalarFetch ft;
  ft.add(res.p, 2, h);
  ft.run();
  std::memcpy(out, &h[0], sizeof(double));
  return true;
}

// ------------------------------------------------------------------ complex dot and trace of a slab-form matrix
// (complex TRS2 steps: DotMatrix = sum conj(a) b, MatrixTrace = sum of the real parts of the diagonal)
namespace {
// one wave per column j of the complex slab-form A: (Re, Im) of sum_r conj(A(r, j)) B(r, j) into dpart[2 j], (Re A(j + col_offset,
// j), 0) into tpart[2 j].  B in complex slab form (BSLAB) or in packed compressed columns (a Hamiltonian that never entered
// slab form); B == nullptr: the trace only.  Fixed shapes (a wave sum per column, then sum_pairs_async): reproducible sums.
template <bool BSLAB>
__global__ __launch_bounds__(256) void k_sa_dot_trace_c(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                        const int64_t* __restrict__ offa, const double2* __restrict__ va,
                                                        const int32_t* __restrict__ fb, const int32_t* __restrict__ lb,
                                                        const int64_t* __restrict__ offb, const double2* __restrict__ vb, Csc bc,
                                                        int col_offset, double* __restrict__ dpart, double* __restrict__ tpart) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int f = fa[j], l = la[j];
  const double2* __restrict__ pa = va + (offa[j] - f);   // (row r of column j at pa[r], r in [f, l])
  double sr = 0.0, si = 0.0;
  if (dpart && l >= f) {
    if constexpr (BSLAB) {
      const int g0 = max(f, fb[j]), g1 = min(l, lb[j]);
      if (g1 >= g0) {
        const double2* __restrict__ pb = vb + (offb[j] - fb[j]);
        for (int r = g0 + lane; r <= g1; r += WAVE) {
          const double2 a = pa[r], b = pb[r];
          sr = __dadd_rn(sr, __dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)));
          si = __dadd_rn(si, __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x)));
        }
      }
    } else {
      const double2* __restrict__ bv = reinterpret_cast<const double2*>(bc.val);
      for (int64_t p = bc.outer[j] + lane, e = bc.outer[j + 1]; p < e; p += WAVE) {
        const int r = bc.inner[p];
        if (r < f || r > l) continue;
        const double2 a = pa[r], b = bv[p];
        sr = __dadd_rn(sr, __dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)));
        si = __dadd_rn(si, __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x)));
      }
    }
  }
  if (dpart) {
    sr = wave_sum_f64(sr);
    si = wave_sum_f64(si);
  }
  if (lane == 0) {
    if (dpart) { dpart[2 * (size_t)j] = sr; dpart[2 * (size_t)j + 1] = si; }
    const int d = j + col_offset;
    tpart[2 * (size_t)j] = (l >= f && d >= f && d <= l) ? pa[d].x : 0.0;
    tpart[2 * (size_t)j + 1] = 0.0;
  }
}
}  // namespace

bool slab_dot_trace_c(const DevMat& A, const DevMat* B, int32_t col_offset, double dot[2], double* trace) {
  // (read-only views of operands with stored zeros are read as they are: a stored zero adds an exact zero to either sum)
  auto view_ok = [](const DevMat& M) { return !M.slab->origin || (options().stored_zero_views != 0 && M.slab->zlast.p != nullptr); };
  if (!A.expanded() || !A.cplx || A.slab->labelled() || !view_ok(A)) return false;
  if (B) {
    if (!B->cplx || B->cols != A.cols || B->rows != A.rows || B->blocked() || B->loose()) return false;
    if (B->expanded() && (B->slab->labelled() || !view_ok(*B))) return false;
  }
  const SlabForm& fa = *A.slab;
  const int n = A.cols;
  const bool bslab = B && B->expanded();
  DevBuf<double> dpart(B ? (size_t)2 * n : 2), tpart((size_t)2 * n), res(4);
  const SlabForm* fb = bslab ? B->slab.get() : nullptr;
  const Csc bc = (B && !bslab) ? view(*B) : Csc{0, 0, nullptr, nullptr, nullptr};
  const double2* va = reinterpret_cast<const double2*>(fa.val.p);
  auto go = [&](auto slab_tag) {
    constexpr bool S = decltype(slab_tag)::value;
    hipLaunchKernelGGL((k_sa_dot_trace_c<S>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p, va,
                       fb ? fb->first.p : nullptr, fb ? fb->last.p : nullptr, fb ? fb->off.p : nullptr,
                       fb ? reinterpret_cast<const double2*>(fb->val.p) : nullptr, bc, col_offset, B ? dpart.p : nullptr, tpart.p);
  };
  if (bslab) go(std::true_type{});
  else go(std::false_type{});
  if (B) sum_pairs_async(dpart.p, n, res.p);
  sum_pairs_async(tpart.p, n, res.p + 2);
  unsigned long long h[4] = {0, 0, 0, 0};
  ScalarFetch ft;
  ft.add(res.p + (B ? 0 : 2), B ? 4 : 2, B ? h : h + 2);
  ft.run();
  double d[4];
  std::memcpy(d, h, sizeof(d));
  if (B) { dot[0] = d[0]; dot[1] = d[1]; }
  if (trace) *trace = d[2];
  return true;
}

// ------------------------------------------------------------------ the recurrence step of the polynomial loops, complex
// Chebyshev and Hermite evaluation do two merges behind every product P: Tk = P + a Tkm2 (IncrementMatrix(Tkm2, P, a)) and
// R <- R + c Tk (IncrementMatrix(Tk, R, c)), both at threshold 0.  One pass per column does both: P, Tkm2 and R are read
// once, Tk and the new R are written once.  Element for element the arithmetic and the keep / drop decisions are those of
// k_sa_axpby<double2, true> (kernels.hip) called twice with beta = 1 and threshold 0 -- the scaled addend rounded, then
// added; a sum that cancels exactly is dropped -- so the two results are those of the two calls bit for bit.
namespace {
// one element of IncrementMatrix(A, B, alpha, 0) on runs: a, b the operands' values at row r (zero: no entry), amax / bmax the
// last rows of A's / B's runs (-1: empty).  The keep rules are k_sa_axpby's own expressions at thr = 0 and beta = 1 (b is its own
// scaled value), so that the two kernels decide alike on every input, non-finite sums included.  keep && zero result: an addend that underflowed
// beyond the other run's end, which the slab form cannot hold (k_sa_axpby's stat bit 1).
__device__ inline double2 step_merge(double2 a, double2 b, double alpha, int r, int amax, int bmax, bool& keep) {
  const bool ha = !Sc<double2>::is_zero(a), hb = !Sc<double2>::is_zero(b);
  const double2 wa = Sc<double2>::scale(alpha, a);
  double2 o = Sc<double2>::zero();
  keep = false;
  if (ha && hb) { o = Sc<double2>::add(wa, b); keep = Sc<double2>::mag(o) > 0.0; }
  else if (ha) { o = wa; keep = (r > bmax) ? true : (Sc<double2>::mag(wa) > 0.0); }
  else if (hb) { o = b; keep = (r > amax) ? true : (Sc<double2>::mag(b) > 0.0); }
  return o;
}
// slots of the two results per column: Tk's is the aligned hull of P's and Tkm2's extents, R's the aligned hull of its old
// extent and Tk's slot
__global__ void k_sa_step_span(const int32_t* __restrict__ fp, const int32_t* __restrict__ lp, const int32_t* __restrict__ fq,
                               const int32_t* __restrict__ lq, const int32_t* __restrict__ fr, const int32_t* __restrict__ lr, int n, int al,
                               int32_t* __restrict__ span_t, int32_t* __restrict__ span_r) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
  if (lp[j] >= fp[j]) { f = fp[j]; l = lp[j]; }
  if (lq[j] >= fq[j]) { f = min(f, fq[j]); l = max(l, lq[j]); }
  int a0 = 0, a1 = 0;
  if (l >= f) { a0 = f / al * al; a1 = (l / al + 1) * al; }
  span_t[j] = a1 - a0;
  if (lr[j] >= fr[j]) {
    const int b0 = fr[j] / al * al, b1 = (lr[j] / al + 1) * al;
    if (a1 > a0) { a0 = min(a0, b0); a1 = max(a1, b1); }
    else { a0 = b0; a1 = b1; }
  }
  span_r[j] = a1 - a0;
}
// One wave per column.  Lane i takes the rows = i (mod 64) in both loops, so the Tk values the second loop reads back are
// the lane's own stores (rows outside Tk's kept extent read as zero without a load).  16-byte loads and stores, consecutive
// lanes on consecutive rows of a run.  stat[0] |= 1: a kept zero (see step_merge), |= 2: a slot beyond its buffer (runs far
// apart: nothing is written for that column) -- the host then declines and the caller's operands are as they were.
__global__ __launch_bounds__(256) void k_sa_recurrence_step_c(
    int n, const int32_t* __restrict__ fp, const int32_t* __restrict__ lp, const int64_t* __restrict__ offp, const double2* __restrict__ vp,
    const int32_t* __restrict__ fq, const int32_t* __restrict__ lq, const int64_t* __restrict__ offq, const double2* __restrict__ vq,
    const int32_t* __restrict__ fr, const int32_t* __restrict__ lr, const int64_t* __restrict__ offr, const double2* __restrict__ vr,
    const int64_t* __restrict__ base_t, const int64_t* __restrict__ base_r, int al, double a, double c, double2* out_t,
    double2* __restrict__ out_r, int32_t* __restrict__ tfirst, int32_t* __restrict__ tlast, int32_t* __restrict__ tcount,
    int64_t* __restrict__ toff, int32_t* __restrict__ rfirst, int32_t* __restrict__ rlast, int32_t* __restrict__ rcount,
    int64_t* __restrict__ roff, unsigned long long* __restrict__ stat, int64_t bound_t, int64_t bound_r) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fP = fp[j], lP = lp[j], fQ = fq[j], lQ = lq[j], fR = fr[j], lR = lr[j];
  const bool anyP = lP >= fP, anyQ = lQ >= fQ, anyR = lR >= fR;
  const int64_t slot_t = base_t[j], slot_r = base_r[j];
  // Tk's slot [t0, t1), R's slot [r0, r1) (k_sa_step_span)
  int t0 = 0, t1 = 0;
  if (anyP || anyQ) {
    const int f = anyP ? (anyQ ? min(fP, fQ) : fP) : fQ, l = anyP ? (anyQ ? max(lP, lQ) : lP) : lQ;
    t0 = f / al * al;
    t1 = (l / al + 1) * al;
  }
  int r0 = t0, r1 = t1;
  if (anyR) {
    const int b0 = fR / al * al, b1 = (lR / al + 1) * al;
    if (t1 > t0) { r0 = min(t0, b0); r1 = max(t1, b1); }
    else { r0 = b0; r1 = b1; }
  }
  if (slot_t + (int64_t)(t1 - t0) > bound_t || slot_r + (int64_t)(r1 - r0) > bound_r) {
    if (lane == 0) {
      tfirst[j] = INT_MAX; tlast[j] = -1; tcount[j] = 0; toff[j] = slot_t;
      rfirst[j] = INT_MAX; rlast[j] = -1; rcount[j] = 0; roff[j] = slot_r;
      atomicOr(stat, 2ull);
    }
    return;
  }
  const double2* __restrict__ pp = anyP ? vp + (offp[j] - fP) : vp;
  const double2* __restrict__ pq = anyQ ? vq + (offq[j] - fQ) : vq;
  const double2* __restrict__ pr = anyR ? vr + (offr[j] - fR) : vr;
  double2* dt = out_t + (slot_t - t0);
  double2* __restrict__ dr = out_r + (slot_r - r0);
  int zk = 0;
  // Tk = P + a Tkm2: IncrementMatrix(Tkm2, P, a)
  int cnt = 0, kf = INT_MAX, kl = -1;
  {
    const int pmax = anyP ? lP : -1, qmax = anyQ ? lQ : -1;
    for (int r = (t0 & ~(WAVE - 1)) + lane; r < t1; r += WAVE) {
      if (r < t0) continue;
      const double2 q = (anyQ && r >= fQ && r <= lQ) ? pq[r] : Sc<double2>::zero();
      const double2 p = (anyP && r >= fP && r <= lP) ? pp[r] : Sc<double2>::zero();
      bool keep;
      const double2 o = step_merge(q, p, a, r, qmax, pmax, keep);
      dt[r] = keep ? o : Sc<double2>::zero();
      zk |= (keep && Sc<double2>::is_zero(o)) ? 1 : 0;
      cnt += keep ? 1 : 0;
      kf = min(kf, keep ? r : INT_MAX);
      kl = max(kl, keep ? r : -1);
    }
    cnt = (int)wave_sum_i64(cnt);
    kf = wave_min_i32(kf);
    kl = wave_max_i32(kl);
    if (lane == 0) {
      tfirst[j] = kf; tlast[j] = kl; tcount[j] = cnt;
      toff[j] = slot_t + (cnt ? kf - t0 : 0);
    }
  }
  // R <- R + c Tk: IncrementMatrix(Tk, R, c), Tk's run is [kf, kl] now
  {
    const bool anyT = kl >= kf;
    const int rmax = anyR ? lR : -1, tmax = anyT ? kl : -1;
    int rc = 0, rf = INT_MAX, rl = -1;
    for (int r = (r0 & ~(WAVE - 1)) + lane; r < r1; r += WAVE) {
      if (r < r0) continue;
      const double2 t = (anyT && r >= kf && r <= kl) ? dt[r] : Sc<double2>::zero();
      const double2 b = (anyR && r >= fR && r <= lR) ? pr[r] : Sc<double2>::zero();
      bool keep;
      const double2 o = step_merge(t, b, c, r, tmax, rmax, keep);
      dr[r] = keep ? o : Sc<double2>::zero();
      zk |= (keep && Sc<double2>::is_zero(o)) ? 1 : 0;
      rc += keep ? 1 : 0;
      rf = min(rf, keep ? r : INT_MAX);
      rl = max(rl, keep ? r : -1);
    }
    rc = (int)wave_sum_i64(rc);
    rf = wave_min_i32(rf);
    rl = wave_max_i32(rl);
    if (lane == 0) {
      rfirst[j] = rf; rlast[j] = rl; rcount[j] = rc;
      roff[j] = slot_r + (rc ? rf - r0 : 0);
    }
  }
  if (__ballot(zk != 0) && lane == 0) atomicOr(stat, 1ull);
}
}  // namespace

// Tk = P + a Tkm2 and R <- R + c Tk on complex matrices in slab form (or column panels of them), what
// slab_axpby_c(Tkm2, P, a, 1, 0) and slab_axpby_c(Tk, R, c, 1, 0) leave behind; Tk may be P.  false: not taken (whatever one
// of the two calls would decline), nothing changed.
bool slab_recurrence_step_c(const DevMat& P, const DevMat& Tkm2, DevMat& Tk, DevMat& R, double a, double c) {
  if (!sa_operand_c(P) || !sa_operand_c(Tkm2) || !sa_operand_c(R)) return false;
  if (P.cols != Tkm2.cols || P.cols != R.cols || P.rows != Tkm2.rows || P.rows != R.rows) return false;
  if (&P == &Tkm2 || &P == &R || &Tkm2 == &R || &Tk == &R || &Tk == &Tkm2) return false;
  if (a == 0.0 || c == 0.0 || P.zero_free != 1 || Tkm2.zero_free != 1 || R.zero_free != 1) return false;
  const SlabForm &sp = *P.slab, &sq = *Tkm2.slab, &sr = *R.slab;
  const int n = P.cols;
  const int al = std::max(sp.row_pad, std::max(sq.row_pad, sr.row_pad));
  if (al % sp.row_pad != 0 || al % sq.row_pad != 0 || al % sr.row_pad != 0) return false;
  // (the buffers of the two merges: the operands' slots and the padding of a union per column)
  const int64_t bound_t = sp.slots + sq.slots + 2LL * al * n, bound_r = bound_t + sr.slots + 2LL * al * n;
  std::unique_ptr<SlabForm> ft(new SlabForm()), fr(new SlabForm());
  for (SlabForm* f : {ft.get(), fr.get()}) {
    f->first.alloc((size_t)n); f->last.alloc((size_t)n); f->count.alloc((size_t)n); f->off.alloc((size_t)n + 1);
  }
  DevBuf<int32_t> span_t((size_t)n), span_r((size_t)n);
  DevBuf<int64_t> base_t((size_t)n + 1), base_r((size_t)n + 1);
  DevBuf<unsigned long long> stat(1), tot(2);
  stat.zero();
  tot.zero();
  hipLaunchKernelGGL(k_sa_step_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), sp.first.p, sp.last.p, sq.first.p, sq.last.p, sr.first.p,
                     sr.last.p, n, al, span_t.p, span_r.p);
  scan_i32_async(span_t.p, base_t.p, (int64_t)n);
  scan_i32_async(span_r.p, base_r.p, (int64_t)n);
  ft->val.alloc(((size_t)bound_t + kIndexSlack) * 2);
  fr->val.alloc(((size_t)bound_r + kIndexSlack) * 2);
  hipLaunchKernelGGL(k_sa_recurrence_step_c, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, sp.first.p, sp.last.p, sp.off.p,
                     reinterpret_cast<const double2*>(sp.val.p), sq.first.p, sq.last.p, sq.off.p, reinterpret_cast<const double2*>(sq.val.p),
                     sr.first.p, sr.last.p, sr.off.p, reinterpret_cast<const double2*>(sr.val.p), base_t.p, base_r.p, al, a, c,
                     reinterpret_cast<double2*>(ft->val.p), reinterpret_cast<double2*>(fr->val.p), ft->first.p, ft->last.p, ft->count.p,
                     ft->off.p, fr->first.p, fr->last.p, fr->count.p, fr->off.p, stat.p, bound_t, bound_r);
  const dim3 sum_grid(std::max(1, std::min(256, cdiv(n, 1024))));
  hipLaunchKernelGGL(k_sa_count_sum, sum_grid, dim3(256), 0, stream(), ft->count.p, n, tot.p);
  hipLaunchKernelGGL(k_sa_count_sum, sum_grid, dim3(256), 0, stream(), fr->count.p, n, tot.p + 1);
  int64_t nnz[2] = {0, 0}, slots_t = 0, slots_r = 0;
  unsigned long long hs = 0;
  {
    ScalarFetch f;
    f.add(tot.p, 2, nnz);
    f.add(base_t.p + n, 1, &slots_t);
    f.add(base_r.p + n, 1, &slots_r);
    f.add(stat.p, 1, &hs);
    f.run();
  }
  if (hs != 0) return false;
  ft->row_pad = al; ft->slots = slots_t;
  fr->row_pad = al; fr->slots = slots_r;
  DevMat T, S;
  T.rows = P.rows; T.cols = n; T.cplx = true; T.nnz = nnz[0]; T.zero_free = 1;
  T.slab = std::move(ft);
  S.rows = R.rows; S.cols = n; S.cplx = true; S.nnz = nnz[1]; S.zero_free = 1;
  S.slab = std::move(fr);
  bump_matrix_value_epoch();   // (two merges in place, as slab_axpby_c counts them)
  bump_matrix_value_epoch();
  Tk = std::move(T);
  R = std::move(S);
  return true;
}

// ------------------------------------------------------------------ how dense the runs are
namespace {
__global__ __launch_bounds__(256) void k_sa_span_sum(const int32_t* __restrict__ first, const int32_t* __restrict__ last, int n,
                                                     unsigned long long* __restrict__ out) {
  __shared__ long long red[4];
  long long s = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s += last[i] >= first[i] ? last[i] - first[i] + 1 : 0;
  s = wave_sum_i64(s);
  if (lane_id() == 0) red[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long t = red[0] + red[1] + red[2] + red[3];
    if (t) atomicAdd(out, (unsigned long long)t);
  }
}
}  // namespace

// rows covered by the runs of a slab-form matrix (kept in the form: its extents never change)
int64_t slab_span_sum(const DevMat& M) {
  if (!M.expanded()) return 0;
  const SlabForm& f = *M.slab;
  if (f.span_sum >= 0) return f.span_sum;
  DevBuf<unsigned long long> acc(1);
  acc.zero();
  hipLaunchKernelGGL(k_sa_span_sum, dim3(std::max(1, std::min(256, cdiv(M.cols, 1024)))), dim3(256), 0, stream(), f.first.p, f.last.p, M.cols,
                     acc.p);
  unsigned long long h = 0;
  ScalarFetch ft;
  ft.add(acc.p, 1, &h);
  ft.run();
  f.span_sum = (int64_t)h;
  return f.span_sum;
}

// ------------------------------------------------------------------ PM purification on a slab-form iterate
// DensityMatrixSolversModule.F90:145-200 per iteration, after the two products X2 = X X and X3 = X X2:
//   CopyMatrix(X, Temp); IncrementMatrix(X2, Temp, -1, thr); trace(Temp), dot(Temp, X)                      (the sigma pass)
//   ScaleMatrix(X, a1); IncrementMatrix(X2, X, a2, thr); IncrementMatrix(X3, X, a3, thr)                    (the update)
// Whenever sigma > 1/2 the update scales X by a1 = 0: compressed columns then hold STORED ZEROS, and AddSparseVectors copies
// the tail of a column beyond the other operand's last row unfiltered -- a stored zero there survives the merge and its
// row steers the tail rule of the merges that follow.  The runs of a slab form read a zero as "no entry", so those rows
// travel in a ZeroList next to zero-free runs.  "Present" below: a non-zero of the run or a row of the list; exh = last
// present row of a column.  Element arithmetic: __dmul_rn / __dadd_rn in the order of the vocabulary calls.
// T = double2 (option complex_pm): runs of (re, im) pairs -- off, the slots, base and bound count pairs.  Every scalar of the loop
// is real, so scalings and sums work part by part (Sc<double2>::scale / add); an entry is a non-zero where either part is, a stored
// zero where both are zero; the threshold is on the modulus, Sc<double2>::mag, the function the merge on compressed columns calls
// (kernels.hip inc_decide), so the kept pattern is that merge's.
namespace {
struct PmRuns {   // the runs of one slab-form operand (val: entries of T)
  const int32_t* __restrict__ first;
  const int32_t* __restrict__ last;
  const int64_t* __restrict__ off;
  const double* __restrict__ val;
};
PmRuns pm_runs(const DevMat& M) { return PmRuns{M.slab->first.p, M.slab->last.p, M.slab->off.p, M.slab->val.p}; }
template <typename T>
struct PmCol {    // one column of it: rows f .. l (l < f: empty) at p[r]
  int f, l;
  const T* __restrict__ p;
  __device__ T at(int r) const { return (r >= f && r <= l) ? p[r] : Sc<T>::zero(); }
};
template <typename T>
__device__ inline PmCol<T> pm_col(const PmRuns& m, int j) {
  PmCol<T> c;
  const T* __restrict__ v = reinterpret_cast<const T*>(m.val);
  c.f = m.first[j]; c.l = m.last[j];
  c.p = c.l >= c.f ? v + (m.off[j] - c.f) : v;
  if (c.l < c.f) { c.f = INT_MAX; c.l = -1; }
  return c;
}
// the term of a dot one row adds: o w, and for complex operands the real part of conj(o) w with each product and the pair's sum
// rounded (the terms of k_sa_dot_trace_c)
__device__ inline double hpcp_term(double o, double w) { return __dmul_rn(o, w); }
__device__ inline double hpcp_term(double2 o, double2 w) { return __dadd_rn(__dmul_rn(o.x, w.x), __dmul_rn(o.y, w.y)); }
// row r among the (few, ascending) listed rows zrow[z0 .. z1) of the column: the loop is uniform over the wave
__device__ inline bool pm_listed(const int32_t* __restrict__ zrow, int64_t z0, int64_t z1, int r) {
  bool in = false;
  for (int64_t q = z0; q < z1; ++q) in |= zrow[q] == r;
  return in;
}
// one row of o = alpha a + b by the AddSparseVectors rules (kernels.hip inc_decide): ha / hb = present, wa = alpha a and b as they
// enter the sum, amax / bmax = last present row of the column of a / of b.  Returns "kept"; *o = the value (may be exactly zero
// where a tail is copied unfiltered)
template <typename T>
__device__ inline bool pm_merge(bool ha, bool hb, T wa, T b, int r, int amax, int bmax, double thr, T* o) {
  if (ha && hb) { *o = Sc<T>::add(wa, b); return Sc<T>::mag(*o) > thr; }
  if (ha) { *o = wa; return (r > bmax) ? true : (Sc<T>::mag(wa) > thr); }
  if (hb) { *o = b; return (r > amax) ? true : (Sc<T>::mag(b) > thr); }
  *o = Sc<T>::zero();
  return false;
}
// part[2 j] = trace, part[2 j + 1] = dot(., X) of column j of Temp = X - X2 (merged at thr), Temp itself not formed (complex: the real
// part of the diagonal entry, as MatrixTrace sums it, and the real part of DotMatrix(Temp, X): hpcp_term)
template <typename T>
__global__ __launch_bounds__(256) void k_pm_sigma(int n, PmRuns X, const int64_t* __restrict__ zoff, const int32_t* __restrict__ zrow,
                                                  PmRuns X2, int col_offset, int al, double thr, double* __restrict__ part) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id(), dg = j + col_offset;
  const PmCol<T> cx = pm_col<T>(X, j), c2 = pm_col<T>(X2, j);
  const int64_t z0 = zoff ? zoff[j] : 0, z1 = zoff ? zoff[j + 1] : 0;
  const int exhx = max(cx.l, z1 > z0 ? zrow[z1 - 1] : -1);
  // (a listed row outside both runs merges to an exact zero: it adds nothing to either sum)
  const int lo = min(cx.f, c2.f), hi = max(cx.l, c2.l);
  double st = 0.0, sd = 0.0;
  if (hi >= lo) {
    const int r0 = lo / al * al, r1 = (hi / al + 1) * al;
    for (int r = r0 + lane; r < r1; r += WAVE) {
      const T x = cx.at(r), x2 = c2.at(r);
      const bool px = !Sc<T>::is_zero(x) || pm_listed(zrow, z0, z1, r);
      T o;
      const bool keep = pm_merge<T>(!Sc<T>::is_zero(x2), px, Sc<T>::scale(-1.0, x2), x, r, c2.l, exhx, thr, &o);
      if (keep) {
        if (r == dg) st = __dadd_rn(st, Sc<T>::re(o));
        sd = __dadd_rn(sd, hpcp_term(o, x));
      }
    }
  }
  st = wave_sum_f64(st);
  sd = wave_sum_f64(sd);
  if (lane == 0) { part[2 * (size_t)j] = st; part[2 * (size_t)j + 1] = sd; }
}
// aligned union of the three runs per column (0: all empty), the output slot of the update
__global__ void k_pm_span(const int32_t* __restrict__ fa, const int32_t* __restrict__ la, const int32_t* __restrict__ fb,
                          const int32_t* __restrict__ lb, const int32_t* __restrict__ fc, const int32_t* __restrict__ lc, int n, int al,
                          int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
  if (la[j] >= fa[j]) { f = min(f, fa[j]); l = max(l, la[j]); }
  if (lb[j] >= fb[j]) { f = min(f, fb[j]); l = max(l, lb[j]); }
  if (lc[j] >= fc[j]) { f = min(f, fc[j]); l = max(l, lc[j]); }
  span[j] = l >= f ? (l / al + 1) * al - f / al * al : 0;
}
// One wave per column.  Loop 1: Y = a2 X2 + a1 X (kept rows, values may be zero) only to find exh(Y); loop 2: Y again and
// o = a3 X3 + Y.  Columns of up to KC * 64 rows keep x, x2 and x3 in registers between the loops (every load of the column is
// requested before the first use); longer ones read the runs again.  KC = PM_KC for double; PM_KC_C for double2, one 16-byte load
// per lane and operand: the same twelve doubles of x, x2 and x3 per lane between the loops.
// MODE 0: kept non-zeros into the slot at base[j] (row r at base + r - a0, pads and dropped rows zero), first / last / count / offset
//         as k_sa_axpby writes them; zcnt[j] = kept rows whose value is exactly zero.  stat |= 2: a union extent beyond the output.
// MODE 1: those rows, ascending, to zout[nzoff[j] ...] (columns with none return at once).
constexpr int PM_KC = 4;
constexpr int PM_KC_C = 2;
template <typename T, int MODE, int KC>
__global__ __launch_bounds__(256) void k_pm_update(int n, PmRuns X, const int64_t* __restrict__ zoff, const int32_t* __restrict__ zrow,
                                                   PmRuns X2, PmRuns X3, double a1, double a2, double a3, double thr, int al,
                                                   const int64_t* __restrict__ base, T* __restrict__ out, int32_t* __restrict__ ofirst,
                                                   int32_t* __restrict__ olast, int32_t* __restrict__ ocount, int64_t* __restrict__ ooff,
                                                   int32_t* __restrict__ zcnt, const int64_t* __restrict__ nzoff, int32_t* __restrict__ zout,
                                                   int64_t bound, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  int64_t zdst = 0;
  if (MODE == 1) {
    zdst = nzoff[j];
    if (nzoff[j + 1] == zdst) return;
  }
  const PmCol<T> cx = pm_col<T>(X, j), c2 = pm_col<T>(X2, j), c3 = pm_col<T>(X3, j);
  const int64_t z0 = zoff ? zoff[j] : 0, z1 = zoff ? zoff[j + 1] : 0;
  const int zf = z1 > z0 ? zrow[z0] : INT_MAX, zl = z1 > z0 ? zrow[z1 - 1] : -1;
  const int exhx = max(cx.l, zl);
  const int f = min(cx.f, min(c2.f, c3.f)), l = max(cx.l, max(c2.l, c3.l));   // the runs: where a non-zero can come out
  const int a0 = l >= f ? f / al * al : 0, a1r = l >= f ? (l / al + 1) * al : 0;
  const int64_t slot = MODE == 0 ? base[j] : 0;
  if (MODE == 0) {
    // (runs that lie far apart: the union is not bounded by the operands' slots -- nothing is written, the host refuses)
    const int own = (cx.l >= cx.f ? (cx.l / al + 1) * al - cx.f / al * al : 0) + (c2.l >= c2.f ? (c2.l / al + 1) * al - c2.f / al * al : 0) +
                    (c3.l >= c3.f ? (c3.l / al + 1) * al - c3.f / al * al : 0);
    if (a1r - a0 > own + 2 * al || slot + (int64_t)(a1r - a0) > bound) {
      if (lane == 0) { ofirst[j] = INT_MAX; olast[j] = -1; ocount[j] = 0; ooff[j] = slot; zcnt[j] = 0; atomicOr(stat, 2ull); }
      return;
    }
  }
  const int lo = min(f, zf), hi = max(l, zl);   // the rows to walk: the runs and the listed rows
  if (hi < lo) {
    if (MODE == 0 && lane == 0) { ofirst[j] = INT_MAX; olast[j] = -1; ocount[j] = 0; ooff[j] = slot; zcnt[j] = 0; }
    return;
  }
  const int r0 = lo / al * al, r1 = (hi / al + 1) * al;
  const bool fits = r1 - r0 <= KC * WAVE;
  T vx[KC], v2[KC], v3[KC];
  unsigned pm = 0;   // bit c: the row of chunk c is present in X
  int ey = -1;
  if (fits) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int r = r0 + c * WAVE + lane;
      const bool in = r < r1;
      vx[c] = in ? cx.at(r) : Sc<T>::zero();
      v2[c] = in ? c2.at(r) : Sc<T>::zero();
      v3[c] = in ? c3.at(r) : Sc<T>::zero();
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int r = r0 + c * WAVE + lane;
      const bool px = r < r1 && (!Sc<T>::is_zero(vx[c]) || pm_listed(zrow, z0, z1, r));
      pm |= px ? (1u << c) : 0u;
      T y;
      if (pm_merge<T>(!Sc<T>::is_zero(v2[c]), px, Sc<T>::scale(a2, v2[c]), Sc<T>::scale(a1, vx[c]), r, c2.l, exhx, thr, &y)) ey = max(ey, r);
    }
  } else {
    for (int r = r0 + lane; r < r1; r += WAVE) {
      const T x = cx.at(r), x2 = c2.at(r);
      const bool px = !Sc<T>::is_zero(x) || pm_listed(zrow, z0, z1, r);
      T y;
      if (pm_merge<T>(!Sc<T>::is_zero(x2), px, Sc<T>::scale(a2, x2), Sc<T>::scale(a1, x), r, c2.l, exhx, thr, &y)) ey = max(ey, r);
    }
  }
  ey = wave_max_i32(ey);
  T* __restrict__ dst = MODE == 0 ? out + (slot - a0) : out;
  int cnt = 0, kf = INT_MAX, kl = -1, nz = 0;
  // one chunk of 64 rows of loop 2 (every lane of the wave comes here: MODE 1 orders its rows with a ballot)
  auto row2 = [&](int r, bool in, T x, bool px, T x2, T x3) {
    T y, o;
    const bool py = in && pm_merge<T>(!Sc<T>::is_zero(x2), px, Sc<T>::scale(a2, x2), Sc<T>::scale(a1, x), r, c2.l, exhx, thr, &y);
    const bool keep = in && pm_merge<T>(!Sc<T>::is_zero(x3), py, Sc<T>::scale(a3, x3), py ? y : Sc<T>::zero(), r, c3.l, ey, thr, &o);
    const bool kz = keep && Sc<T>::is_zero(o), kv = keep && !Sc<T>::is_zero(o);
    if (MODE == 0) {
      if (in && r >= a0 && r < a1r) dst[r] = kv ? o : Sc<T>::zero();
      cnt += kv ? 1 : 0;
      nz += kz ? 1 : 0;
      kf = min(kf, kv ? r : INT_MAX);
      kl = max(kl, kv ? r : -1);
    } else {
      const unsigned long long m = __ballot(kz);
      if (kz) zout[zdst + nz + __popcll(m & lanemask_lt())] = r;
      nz += __popcll(m);
    }
  };
  if (fits) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int r = r0 + c * WAVE + lane;
      row2(r, r < r1, vx[c], (pm >> c) & 1u, v2[c], v3[c]);
    }
  } else {
    for (int rb = r0; rb < r1; rb += WAVE) {
      const int r = rb + lane;
      const bool in = r < r1;
      const T x = in ? cx.at(r) : Sc<T>::zero();
      row2(r, in, x, in && (!Sc<T>::is_zero(x) || pm_listed(zrow, z0, z1, r)), in ? c2.at(r) : Sc<T>::zero(), in ? c3.at(r) : Sc<T>::zero());
    }
  }
  if (MODE == 0) {
    cnt = (int)wave_sum_i64(cnt);
    nz = (int)wave_sum_i64(nz);
    kf = wave_min_i32(kf);
    kl = wave_max_i32(kl);
    if (lane == 0) {
      ofirst[j] = kf; olast[j] = kl; ocount[j] = cnt; zcnt[j] = nz;
      ooff[j] = slot + (cnt ? kf - a0 : 0);
    }
  }
}
// zero-free slab forms of one kind, one alignment and one shape (complex: runs of (re, im) pairs in slots of 16 rows, no view)
bool pm_operands(bool cplx, const DevMat& X, const DevMat& X2, const DevMat* X3) {
  auto pair = [cplx](const DevMat& A, const DevMat& B) { return cplx ? trs4_operands_c(A, B) : trs4_operands(A, B); };
  if (!pair(X, X2)) return false;
  return !X3 || (pair(X, *X3) && X.rows == X3->rows);
}
// column j of Out = column j of A with the rows zrow[zoff[j] ..) inserted as stored zeros (both ascending and disjoint); T = double2:
// stored (0, 0) entries
template <typename T>
__global__ __launch_bounds__(256) void k_insert_zeros(Csc A, const int64_t* __restrict__ zoff, const int32_t* __restrict__ zrow,
                                                      int64_t* __restrict__ oouter, int32_t* __restrict__ oinner, T* __restrict__ oval) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= A.cols) return;
  const int lane = lane_id();
  const int64_t as = A.outer[j], ae = A.outer[j + 1], z0 = zoff[j], z1 = zoff[j + 1], dst = as + z0;
  const T* __restrict__ av = static_cast<const T*>(A.val);
  for (int64_t p = as + lane; p < ae; p += WAVE) {
    const int r = A.inner[p];
    int k = 0;
    for (int64_t q = z0; q < z1; ++q) k += zrow[q] < r ? 1 : 0;
    oinner[dst + (p - as) + k] = r;
    oval[dst + (p - as) + k] = av[p];
  }
  for (int64_t q = z0 + lane; q < z1; q += WAVE) {
    const int r = zrow[q];
    int64_t a = as, b = ae;   // entries of the column below row r
    while (a < b) {
      const int64_t m = (a + b) / 2;
      if (A.inner[m] < r) a = m + 1;
      else b = m;
    }
    oinner[dst + (q - z0) + (a - as)] = r;
    oval[dst + (q - z0) + (a - as)] = Sc<T>::zero();
  }
  if (lane == 0) {
    oouter[j] = dst;
    if (j == A.cols - 1) oouter[j + 1] = ae + z1;
  }
}
// the two passes on operands of one kind
template <typename T>
bool pm_sigma_run(const DevMat& X, const ZeroList& Z, const DevMat& X2, double thr, int32_t col_offset, double out2[2]) {
  if (!pm_operands(Sc<T>::cplx, X, X2, nullptr)) return false;
  const int n = X.cols;
  DevBuf<double> part((size_t)2 * n);
  hipLaunchKernelGGL(k_pm_sigma<T>, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, pm_runs(X), Z.count ? Z.off.p : nullptr,
                     Z.row.p, pm_runs(X2), col_offset, std::max(1, X.slab->row_pad), thr, part.p);
  fetch_pair_sums(part, n, out2);
  return true;
}
// (the slots, `bound` and the output's buffer count entries of T)
template <typename T, int KC>
bool pm_update_run(const DevMat& X, const ZeroList& Z, const DevMat& X2, const DevMat& X3, double a1, double a2, double a3, double thr,
                   DevMat& Out, ZeroList& Zout) {
  constexpr bool cplx = Sc<T>::cplx;
  if (!pm_operands(cplx, X, X2, &X3)) return false;
  const SlabForm &fx = *X.slab, &f2 = *X2.slab, &f3 = *X3.slab;
  const int n = X.cols, al = std::max(1, fx.row_pad);
  std::unique_ptr<SlabForm> fo(new SlabForm());
  fo->first.alloc((size_t)n); fo->last.alloc((size_t)n); fo->count.alloc((size_t)n); fo->off.alloc((size_t)n + 1);
  DevBuf<int32_t> span((size_t)n), zcnt((size_t)n);
  DevBuf<int64_t> base((size_t)n + 1);
  ZeroList zn;
  zn.off.alloc((size_t)n + 1);
  hipLaunchKernelGGL(k_pm_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), fx.first.p, fx.last.p, f2.first.p, f2.last.p, f3.first.p, f3.last.p,
                     n, al, span.p);
  scan_i32_async(span.p, base.p, (int64_t)n);
  // (a column's slot is at most its operands' three slots and two pads: what the kernel refuses beyond)
  const int64_t bound = fx.slots + f2.slots + f3.slots + 2LL * al * n;
  fo->val.alloc(((size_t)bound + kIndexSlack) * (cplx ? 2 : 1));
  DevBuf<unsigned long long> stat(1), tot(1);
  stat.zero();
  tot.zero();
  const int64_t* zoff = Z.count ? Z.off.p : nullptr;
  const dim3 grid(cdiv((int64_t)n * WAVE, 256));
  hipLaunchKernelGGL((k_pm_update<T, 0, KC>), grid, dim3(256), 0, stream(), n, pm_runs(X), zoff, Z.row.p, pm_runs(X2), pm_runs(X3), a1, a2, a3, thr,
                     al, base.p, reinterpret_cast<T*>(fo->val.p), fo->first.p, fo->last.p, fo->count.p, fo->off.p, zcnt.p, (const int64_t*)nullptr, (int32_t*)nullptr,
                     bound, stat.p);
  scan_i32_async(zcnt.p, zn.off.p, (int64_t)n);
  hipLaunchKernelGGL(k_sa_count_sum, dim3(std::max(1, std::min(256, cdiv(n, 1024)))), dim3(256), 0, stream(), fo->count.p, n, tot.p);
  int64_t nnz = 0, slots = 0, nzero = 0;
  unsigned long long hs = 0;
  {
    ScalarFetch ft;
    ft.add(tot.p, 1, &nnz);
    ft.add(base.p + n, 1, &slots);
    ft.add(zn.off.p + n, 1, &nzero);
    ft.add(stat.p, 1, &hs);
    ft.run();
  }
  if (hs != 0) return false;
  if (nzero > 0) {
    zn.row.alloc((size_t)nzero);
    hipLaunchKernelGGL((k_pm_update<T, 1, KC>), grid, dim3(256), 0, stream(), n, pm_runs(X), zoff, Z.row.p, pm_runs(X2), pm_runs(X3), a1, a2, a3,
                       thr, al, (const int64_t*)nullptr, (T*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                       (int64_t*)nullptr, (int32_t*)nullptr, zn.off.p, zn.row.p, bound, (unsigned long long*)nullptr);
  }
  zn.count = nzero;
  fo->row_pad = al;
  fo->slots = slots;
  DevMat R;
  R.rows = X.rows; R.cols = n; R.cplx = cplx; R.nnz = nnz; R.zero_free = 1;
  R.slab = std::move(fo);
  Out = std::move(R);
  Zout = std::move(zn);
  return true;
}
}  // namespace

bool slab_pm_sigma(const DevMat& X, const ZeroList& Z, const DevMat& X2, double thr, int32_t col_offset, double out2[2]) {
  return pm_sigma_run<double>(X, Z, X2, thr, col_offset, out2);
}
bool slab_pm_sigma_c(const DevMat& X, const ZeroList& Z, const DevMat& X2, double thr, int32_t col_offset, double out2[2]) {
  return pm_sigma_run<double2>(X, Z, X2, thr, col_offset, out2);
}
bool slab_pm_update(const DevMat& X, const ZeroList& Z, const DevMat& X2, const DevMat& X3, double a1, double a2, double a3, double thr,
                    DevMat& Out, ZeroList& Zout) {
  return pm_update_run<double, PM_KC>(X, Z, X2, X3, a1, a2, a3, thr, Out, Zout);
}
bool slab_pm_update_c(const DevMat& X, const ZeroList& Z, const DevMat& X2, const DevMat& X3, double a1, double a2, double a3, double thr,
                      DevMat& Out, ZeroList& Zout) {
  return pm_update_run<double2, PM_KC_C>(X, Z, X2, X3, a1, a2, a3, thr, Out, Zout);
}

void insert_stored_zeros(DevMat& M, const ZeroList& Z) {
  if (Z.count == 0) return;
  pack(M);
  DevMat R;
  R.alloc(M.rows, M.cols, M.cplx, M.nnz + Z.count);
  const dim3 grid(cdiv((int64_t)M.cols * WAVE, 256));
  dispatch_type(M.cplx, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_insert_zeros<T>, grid, dim3(256), 0, stream(), view(M), Z.off.p, Z.row.p, R.outer.p, R.inner.p,
                       reinterpret_cast<T*>(R.val.p));
  });
  M = std::move(R);
}

void zero_list_from_pattern(const DevMat& M, ZeroList& Z) {
  Z.clear();
  if (M.nnz == 0) return;
  const Csc v = view(M);
  Z.off.alloc((size_t)M.cols + 1);
  Z.row.alloc((size_t)M.nnz);
  HIP_CHECK(hipMemcpyAsync(Z.off.p, v.outer, sizeof(int64_t) * ((size_t)M.cols + 1), hipMemcpyDeviceToDevice, stream()));
  HIP_CHECK(hipMemcpyAsync(Z.row.p, v.inner, sizeof(int32_t) * (size_t)M.nnz, hipMemcpyDeviceToDevice, stream()));
  Z.count = M.nnz;
}

DevMat zero_list_matrix(const ZeroList& Z, int32_t rows, int32_t cols, bool cplx) {
  DevMat R;
  if (Z.count == 0) { R.reset_empty(rows, cols, cplx); return R; }
  R.alloc(rows, cols, cplx, Z.count);
  HIP_CHECK(hipMemcpyAsync(R.outer.p, Z.off.p, sizeof(int64_t) * ((size_t)cols + 1), hipMemcpyDeviceToDevice, stream()));
  HIP_CHECK(hipMemcpyAsync(R.inner.p, Z.row.p, sizeof(int32_t) * (size_t)Z.count, hipMemcpyDeviceToDevice, stream()));
  HIP_CHECK(hipMemsetAsync(R.val.p, 0, sizeof(double) * (size_t)Z.count * R.wval(), stream()));
  return R;
}

// ------------------------------------------------------------------ the polynomial chain of the square-root step
// NewtonSchultzISRTaylor (SquareRootSolversModule.F90:425-479) builds, between the product X2 = X X and the next product, with
// IncrementMatrix / CopyMatrix / ScaleMatrix at threshold 0 (d = the identity's entry: 1 on the diagonal):
//   order 5:  t = x2 + a x,   u = x + b d,   q = t + u (Temp2),   p = t + c d (Temp)
//   order 3:  y = d + (-1/2) x,   o = 0.375 x2 + y (the new X)
// One pass per column reads X and X2 once and writes the outputs.  Every merge is AddSparseVectors at threshold 0 on two
// operands: both present -> the sum of the two scaled values, each rounded on its own, an exact zero dropped; one present ->
// its scaled value; the result of a merge enters the next one as present iff it was kept.  A scaled value that is exactly zero
// for an entry that is not (an underflow) would be a stored zero of an unfiltered tail or a dropped one-sided entry, depending
// on the other operand's extent: stat |= 1 and the host refuses.  All constants are real: complex operands part by part.
namespace {
__device__ inline double isr_one(double) { return 1.0; }
__device__ inline double2 isr_one(double2) { return make_double2(1.0, 0.0); }
// sa a + sb b of one row; ha / hb: present.  *present: the result is an entry (returned as zero otherwise)
template <typename T>
__device__ inline T isr_merge(double sa, T a, bool ha, double sb, T b, bool hb, bool* present, int* underflow) {
  const T wa = Sc<T>::scale(sa, a), wb = Sc<T>::scale(sb, b);
  *underflow |= ((ha && Sc<T>::is_zero(wa)) || (hb && Sc<T>::is_zero(wb))) ? 1 : 0;
  const T o = ha ? (hb ? Sc<T>::add(wa, wb) : wa) : wb;
  *present = (ha || hb) && Sc<T>::mag(o) > 0.0;
  return *present ? o : Sc<T>::zero();
}
constexpr int ISR_KC = 4;   // chunks of 64 rows whose loads are all requested before the first of them is used
// One wave per column, lanes on consecutive rows of the aligned union [a0, a1) of the two runs and the diagonal row.
// ORDER 5: o1 = Temp2 (q), o2 = Temp (p); ORDER 3: o1 = the new X, s1 = -1/2, s2 = 0.375, o2 unused.
// stat |= 1: an underflow (see above); |= 2: a union extent that the operands' slots do not bound (the two runs far apart, or
// diagonals so far from their runs that the output buffer ends) -- nothing is written for that column.
template <typename T, int ORDER>
__global__ __launch_bounds__(256) void k_sa_isr_chain(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                      const int64_t* __restrict__ offa, const T* __restrict__ va,
                                                      const int32_t* __restrict__ fb, const int32_t* __restrict__ lb,
                                                      const int64_t* __restrict__ offb, const T* __restrict__ vb, int col_offset, double s1,
                                                      double s2, double s3, int al, const int64_t* __restrict__ base, IsrOut o1, IsrOut o2,
                                                      int64_t bound, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = fa[j], lA = la[j], fB = fb[j], lB = lb[j], dg = j + col_offset;
  const bool anyA = lA >= fA, anyB = lB >= fB;
  int f = dg, l = dg;   // (the identity's entry is always there)
  if (anyA) { f = min(f, fA); l = max(l, lA); }
  if (anyB) { f = min(f, fB); l = max(l, lB); }
  const int a0 = f / al * al, a1 = (l / al + 1) * al;
  const int64_t slot = base[j];
  // (the two runs far apart: their union is not bounded by the two slots and two pads -- refused per column, as k_pm_update does.
  // The diagonal row may lie anywhere -- a lone entry of a converged X beside an empty X2 --: what it adds is bounded over all
  // columns by the output buffer, as in k_sa_axpby and k_sa_trs4)
  bool apart = false;
  if (anyA && anyB) {
    const int own = ((lA / al + 1) * al - fA / al * al) + ((lB / al + 1) * al - fB / al * al);
    apart = (max(lA, lB) / al + 1) * al - min(fA, fB) / al * al > own + 2 * al;
  }
  if (apart || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
      o1.first[j] = INT_MAX; o1.last[j] = -1; o1.count[j] = 0; o1.off[j] = slot;
      if (ORDER == 5) { o2.first[j] = INT_MAX; o2.last[j] = -1; o2.count[j] = 0; o2.off[j] = slot; }
      atomicOr(stat, 2ull);
    }
    return;
  }
  const T* __restrict__ pa = anyA ? va + (offa[j] - fA) : va;
  const T* __restrict__ pb = anyB ? vb + (offb[j] - fB) : vb;
  T* __restrict__ d1 = static_cast<T*>(o1.val) + (slot - a0);
  T* __restrict__ d2 = ORDER == 5 ? static_cast<T*>(o2.val) + (slot - a0) : nullptr;
  const T one = isr_one(T{});
  int uf = 0, c1 = 0, f1 = INT_MAX, l1 = -1, c2 = 0, f2 = INT_MAX, l2 = -1;
  for (int rb = a0; rb < a1; rb += ISR_KC * WAVE) {
    T vx[ISR_KC], v2[ISR_KC];
#pragma unroll
    for (int k = 0; k < ISR_KC; ++k) {
      const int r = rb + k * WAVE + lane;
      vx[k] = (anyA && r >= fA && r <= lA) ? pa[r] : Sc<T>::zero();
      v2[k] = (anyB && r >= fB && r <= lB) ? pb[r] : Sc<T>::zero();
    }
#pragma unroll
    for (int k = 0; k < ISR_KC; ++k) {
      const int r = rb + k * WAVE + lane;
      if (r >= a1) continue;
      const T x = vx[k], x2 = v2[k];
      const bool hx = !Sc<T>::is_zero(x), h2 = !Sc<T>::is_zero(x2), hd = r == dg;
      if (ORDER == 5) {
        bool ht, hu, hq, hp;
        const T t = isr_merge<T>(s1, x, hx, 1.0, x2, h2, &ht, &uf);     // IncrementMatrix(X, Temp, a)
        const T u = isr_merge<T>(1.0, x, hx, s2, one, hd, &hu, &uf);    // Temp2 = b I, then IncrementMatrix(X, Temp2)
        const T q = isr_merge<T>(1.0, t, ht, 1.0, u, hu, &hq, &uf);     // IncrementMatrix(Temp, Temp2)
        const T p = isr_merge<T>(s3, one, hd, 1.0, t, ht, &hp, &uf);    // IncrementMatrix(Identity, Temp, c)
        d1[r] = q;
        d2[r] = p;
        c1 += hq ? 1 : 0; f1 = min(f1, hq ? r : INT_MAX); l1 = max(l1, hq ? r : -1);
        c2 += hp ? 1 : 0; f2 = min(f2, hp ? r : INT_MAX); l2 = max(l2, hp ? r : -1);
      } else {
        bool hy, ho;
        const T y = isr_merge<T>(1.0, one, hd, s1, x, hx, &hy, &uf);    // ScaleMatrix(X, -1/2); IncrementMatrix(Identity, X)
        const T o = isr_merge<T>(s2, x2, h2, 1.0, y, hy, &ho, &uf);     // IncrementMatrix(Temp, X, 0.375)
        d1[r] = o;
        c1 += ho ? 1 : 0; f1 = min(f1, ho ? r : INT_MAX); l1 = max(l1, ho ? r : -1);
      }
    }
  }
  c1 = (int)wave_sum_i64(c1);
  f1 = wave_min_i32(f1);
  l1 = wave_max_i32(l1);
  if (ORDER == 5) {
    c2 = (int)wave_sum_i64(c2);
    f2 = wave_min_i32(f2);
    l2 = wave_max_i32(l2);
  }
  if (__ballot(uf != 0) && lane == 0) atomicOr(stat, 1ull);
  if (lane == 0) {
    o1.first[j] = f1; o1.last[j] = l1; o1.count[j] = c1;
    o1.off[j] = slot + (c1 ? f1 - a0 : 0);
    if (ORDER == 5) {
      o2.first[j] = f2; o2.last[j] = l2; o2.count[j] = c2;
      o2.off[j] = slot + (c2 ? f2 - a0 : 0);
    }
  }
}
// trs4_operands, complex operands too (both of one kind)
bool isr_operands(const DevMat& X, const DevMat& X2) {
  auto ok = [](const DevMat& M) {
    return M.expanded() && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1 &&
           (!M.cplx || M.slab->row_pad % 16 == 0);
  };
  const bool take = &X != &X2 && ok(X) && ok(X2) && X.cplx == X2.cplx && X.cols == X2.cols && X.rows == X2.rows && X.slab->row_pad == X2.slab->row_pad;
  if (!take && std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
    std::fprintf(stderr, "[isr chain] operands not taken: slab form %d %d, views %d %d, zero-free %d %d, alignment %d %d\n", (int)X.expanded(),
                 (int)X2.expanded(), X.expanded() && X.slab->origin ? 1 : 0, X2.expanded() && X2.slab->origin ? 1 : 0, X.zero_free, X2.zero_free,
                 X.expanded() ? X.slab->row_pad : -1, X2.expanded() ? X2.slab->row_pad : -1);
  return take;
}
// the chain on X and X2: Out1 (and Out2 in order 5) as fresh slab-form matrices; false: refused, nothing written to them
template <typename T, int ORDER>
bool isr_chain_run(const DevMat& X, const DevMat& X2, double s1, double s2, double s3, int32_t col_offset, DevMat& Out1, DevMat* Out2) {
  const SlabForm &fa = *X.slab, &fb = *X2.slab;
  const int n = X.cols, al = std::max(1, fa.row_pad);
  // (the operands' slots, and per column the diagonal's slot and the pads of a union -- with room for diagonals away from their runs)
  const int64_t bound = fa.slots + fb.slots + 4LL * al * n;
  FreshSlabs fs(n, ORDER == 5 ? 2 : 1, bound, Sc<T>::cplx, false);
  hipLaunchKernelGGL(k_sa_trs4_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), fa.first.p, fa.last.p, fb.first.p, fb.last.p, n, col_offset,
                     al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL((k_sa_isr_chain<T, ORDER>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p,
                     reinterpret_cast<const T*>(fa.val.p), fb.first.p, fb.last.p, fb.off.p, reinterpret_cast<const T*>(fb.val.p), col_offset, s1,
                     s2, s3, al, fs.base.p, fs.out(0), fs.out(1), bound, fs.stat.p);
  DevMat R[2];
  if (!fs.finish("isr chain", X.rows, al, R)) return false;
  bump_matrix_value_epoch();   // (of the calls it replaces, two are merges in place: slab_axpby counts them so)
  bump_matrix_value_epoch();
  Out1 = std::move(R[0]);
  if (ORDER == 5) *Out2 = std::move(R[1]);
  return true;
}
}  // namespace

bool slab_isr_chain5(const DevMat& X, const DevMat& X2, double a, double b, double c, int32_t col_offset, DevMat& Temp2, DevMat& Temp) {
  if (!isr_operands(X, X2) || &Temp2 == &Temp || &Temp2 == &X) return false;
  if (X.cplx) return isr_chain_run<double2, 5>(X, X2, a, b, c, col_offset, Temp2, &Temp);
  return isr_chain_run<double, 5>(X, X2, a, b, c, col_offset, Temp2, &Temp);
}

bool slab_isr_chain3(const DevMat& X, const DevMat& X2, int32_t col_offset, DevMat& Out) {
  if (!isr_operands(X, X2)) return false;
  if (X.cplx) return isr_chain_run<double2, 3>(X, X2, -0.5, 0.375, 0.0, col_offset, Out, nullptr);
  return isr_chain_run<double, 3>(X, X2, -0.5, 0.375, 0.0, col_offset, Out, nullptr);
}

// ------------------------------------------------------------------ HPCP purification: the traces and the update of a step
// DensityMatrixSolversModule.F90:839-878 builds, around the products DDH = D1 DH and D2DH = D1 DDH, with the vocabulary at threshold 0
// (d = the identity's entry):
//   sigma = trace(D2DH) / trace(DDH)
//   t = d1 + 2 d2dh,   o = t + (-2 sigma) ddh (the new D1),   energy = dot(o, wh),   dh = -(o + (-1) d) (the next step's DH)
// k_hpcp_traces leaves both diagonals as the pairs that sum_pairs_async sums member by member: the bits of two slab_trace calls.
// k_hpcp_update reads the three runs and WH once and writes the new D1 and DH; every merge is isr_merge (AddSparseVectors on two
// operands at threshold 0, see the square-root chain above), the scaling by -1 is exact.
namespace {
// one thread per column: part[2 j] = A's diagonal entry, part[2 j + 1] = B's, each read as k_sa_diag reads it; T = double2 (runs of
// (re, im) pairs): the real part, as k_sa_dot_trace_c reads it -- MatrixTrace of a complex matrix sums the real parts
template <typename T>
__global__ __launch_bounds__(256) void k_hpcp_traces(int n, SlabRuns A, SlabRuns B, int col_offset, double* __restrict__ part) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const T* __restrict__ va = reinterpret_cast<const T*>(A.val);
  const T* __restrict__ vb = reinterpret_cast<const T*>(B.val);
  const int d = j + col_offset, fA = A.first[j], lA = A.last[j], fB = B.first[j], lB = B.last[j];
  part[2 * (size_t)j] = (lA >= fA && d >= fA && d <= lA) ? Sc<T>::re(va[A.off[j] + (d - fA)]) : 0.0;
  part[2 * (size_t)j + 1] = (lB >= fB && d >= fB && d <= lB) ? Sc<T>::re(vb[B.off[j] + (d - fB)]) : 0.0;
}
// the aligned hull of the three runs and the diagonal row, per column
__global__ void k_hpcp_span(SlabRuns A, SlabRuns B, SlabRuns C, int n, int col_offset, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = j + col_offset, l = j + col_offset;
  if (A.last[j] >= A.first[j]) { f = min(f, A.first[j]); l = max(l, A.last[j]); }
  if (B.last[j] >= B.first[j]) { f = min(f, B.first[j]); l = max(l, B.last[j]); }
  if (C.last[j] >= C.first[j]) { f = min(f, C.first[j]); l = max(l, C.last[j]); }
  span[j] = (l / al + 1) * al - f / al * al;
}
// chunks of 64 rows whose loads (four operands each) are all requested before the first of them is used: 16 loads per lane in 82
// VGPRs, five waves per SIMD, no scratch -- a hull of up to 256 aligned rows is one trip (ISR_KC's depth with twice the operands)
constexpr int HPCP_KC = 4;
// ... and on runs of (re, im) pairs (option complex_hpcp), one 16-byte load per lane and operand: two chunks in flight are the 32
// VGPRs of load data the real kernel's four are -- 84 VGPRs, five waves per SIMD, no scratch; a hull of up to 128 aligned rows is
// one trip
constexpr int HPCP_KC_C = 2;
// (the term of DotMatrix(D1, WH) one row adds is hpcp_term, above)
__device__ inline double hpcp_negate(double u) { return -u; }   // ScaleMatrix(., -1): exact
__device__ inline double2 hpcp_negate(double2 u) { return Sc<double2>::scale(-1.0, u); }
// One wave per column, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of A = D1, B = DDH, C = D2DH and the
// diagonal row.  o1 = the new D1, o2 = DH, both into the slot at base[j]; part[2 j] = sum over the column of o wh, a lane-strided
// sum then a wave sum (fixed shapes: the same value every run).  s2 = -2 sigma as the host rounds it.
// stat |= 1: a scaled entry underflows to zero; |= 2: runs far apart or a slot beyond the output buffer -- nothing is written for
// that column (k_sa_isr_chain).
// T = double2: the runs, the slots, base and bound count (re, im) pairs; every scalar of the chain is real, so isr_merge<double2>
// scales and adds part by part and keeps an entry where either part is not zero; d = (1, 0).
template <typename T, int KC>
__global__ __launch_bounds__(256) void k_hpcp_update(int n, SlabRuns A, SlabRuns B, SlabRuns C, SlabRuns W, int col_offset, double s2, int al,
                                                     const int64_t* __restrict__ base, IsrOut o1, IsrOut o2, int64_t bound,
                                                     double* __restrict__ part, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = A.first[j], lA = A.last[j], fB = B.first[j], lB = B.last[j], fC = C.first[j], lC = C.last[j], fW = W.first[j], lW = W.last[j];
  const int dg = j + col_offset;
  const bool anyA = lA >= fA, anyB = lB >= fB, anyC = lC >= fC, anyW = lW >= fW;
  int f = dg, l = dg;   // (the identity's entry is always there)
  int rf = INT_MAX, rl = -1, own = 0;   // the hull of the runs alone, and the rows their own aligned slots hold
  if (anyA) { rf = min(rf, fA); rl = max(rl, lA); own += (lA / al + 1) * al - fA / al * al; }
  if (anyB) { rf = min(rf, fB); rl = max(rl, lB); own += (lB / al + 1) * al - fB / al * al; }
  if (anyC) { rf = min(rf, fC); rl = max(rl, lC); own += (lC / al + 1) * al - fC / al * al; }
  if (rl >= 0) { f = min(f, rf); l = max(l, rl); }
  const int a0 = f / al * al, a1 = (l / al + 1) * al;
  const int64_t slot = base[j];
  // (runs far apart: their hull is not bounded by the three slots and the pads between them -- refused per column.  The diagonal
  // row may lie anywhere: what it adds is bounded over all columns by the output buffer)
  const bool apart = rl >= 0 && (rl / al + 1) * al - rf / al * al > own + 3 * al;
  if (apart || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
      o1.first[j] = INT_MAX; o1.last[j] = -1; o1.count[j] = 0; o1.off[j] = slot;
      o2.first[j] = INT_MAX; o2.last[j] = -1; o2.count[j] = 0; o2.off[j] = slot;
      part[2 * (size_t)j] = 0.0; part[2 * (size_t)j + 1] = 0.0;
      atomicOr(stat, 2ull);
    }
    return;
  }
  const T *__restrict__ va0 = reinterpret_cast<const T*>(A.val), *__restrict__ vb0 = reinterpret_cast<const T*>(B.val);
  const T *__restrict__ vc0 = reinterpret_cast<const T*>(C.val), *__restrict__ vw0 = reinterpret_cast<const T*>(W.val);
  const T* __restrict__ pa = anyA ? va0 + (A.off[j] - fA) : va0;
  const T* __restrict__ pb = anyB ? vb0 + (B.off[j] - fB) : vb0;
  const T* __restrict__ pc = anyC ? vc0 + (C.off[j] - fC) : vc0;
  const T* __restrict__ pw = anyW ? vw0 + (W.off[j] - fW) : vw0;
  T* __restrict__ d1 = static_cast<T*>(o1.val) + (slot - a0);
  T* __restrict__ d2 = static_cast<T*>(o2.val) + (slot - a0);
  const T one = isr_one(T{});
  int uf = 0, c1 = 0, f1 = INT_MAX, l1 = -1, c2 = 0, f2 = INT_MAX, l2 = -1;
  double e = 0.0;
  for (int rb = a0; rb < a1; rb += KC * WAVE) {
    T va[KC], vb[KC], vc[KC], vw[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int r = rb + k * WAVE + lane;
      va[k] = (anyA && r >= fA && r <= lA) ? pa[r] : Sc<T>::zero();
      vb[k] = (anyB && r >= fB && r <= lB) ? pb[r] : Sc<T>::zero();
      vc[k] = (anyC && r >= fC && r <= lC) ? pc[r] : Sc<T>::zero();
      vw[k] = (anyW && r >= fW && r <= lW) ? pw[r] : Sc<T>::zero();
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int r = rb + k * WAVE + lane;
      if (r >= a1) continue;
      const T x = va[k], xb = vb[k], xc = vc[k];
      bool ht, ho, hu;
      const T t = isr_merge<T>(1.0, x, !Sc<T>::is_zero(x), 2.0, xc, !Sc<T>::is_zero(xc), &ht, &uf);   // IncrementMatrix(D2DH, D1, 2)
      const T o = isr_merge<T>(1.0, t, ht, s2, xb, !Sc<T>::is_zero(xb), &ho, &uf);                    // IncrementMatrix(DDH, D1, -2 sigma)
      const T u = isr_merge<T>(1.0, o, ho, -1.0, one, r == dg, &hu, &uf);                             // CopyMatrix(D1, DH); IncrementMatrix(I, DH, -1)
      d1[r] = o;
      d2[r] = hu ? hpcp_negate(u) : Sc<T>::zero();                                                    // ScaleMatrix(DH, -1)
      e = __dadd_rn(e, hpcp_term(o, vw[k]));                                                          // DotMatrix(D1, WH)
      c1 += ho ? 1 : 0; f1 = min(f1, ho ? r : INT_MAX); l1 = max(l1, ho ? r : -1);
      c2 += hu ? 1 : 0; f2 = min(f2, hu ? r : INT_MAX); l2 = max(l2, hu ? r : -1);
    }
  }
  c1 = (int)wave_sum_i64(c1);
  f1 = wave_min_i32(f1);
  l1 = wave_max_i32(l1);
  c2 = (int)wave_sum_i64(c2);
  f2 = wave_min_i32(f2);
  l2 = wave_max_i32(l2);
  e = wave_sum_f64(e);
  if (__ballot(uf != 0) && lane == 0) atomicOr(stat, 1ull);
  if (lane == 0) {
    o1.first[j] = f1; o1.last[j] = l1; o1.count[j] = c1;
    o1.off[j] = slot + (c1 ? f1 - a0 : 0);
    o2.first[j] = f2; o2.last[j] = l2; o2.count[j] = c2;
    o2.off[j] = slot + (c2 ? f2 - a0 : 0);
    part[2 * (size_t)j] = e; part[2 * (size_t)j + 1] = 0.0;
  }
}
// what the three merged operands must be: trs4_operands for three
// (cplx: runs of (re, im) pairs in slots aligned to 16 rows, what sa_operand_c takes)
bool hpcp_operand(const DevMat& M, bool cplx = false) {
  return M.expanded() && M.cplx == cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1 &&
         (!cplx || M.slab->row_pad % 16 == 0);
}
template <typename T>
bool hpcp_traces_run(const DevMat& DDH, const DevMat& D2DH, int32_t col_offset, double out2[2]) {
  const int n = DDH.cols;
  DevBuf<double> part((size_t)2 * n);
  hipLaunchKernelGGL(k_hpcp_traces<T>, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, slab_runs(DDH), slab_runs(D2DH), col_offset, part.p);
  fetch_pair_sums(part, n, out2);
  return true;
}
// the update on operands of one kind; the slots, `bound` and the outputs' buffers count entries of T
template <typename T, int KC>
bool hpcp_update_run(const DevMat& D1, const DevMat& DDH, const DevMat& D2DH, double sigma, const DevMat& WH, int32_t col_offset, DevMat& OutD1,
                     DevMat& OutDH, double* energy) {
  constexpr bool cplx = Sc<T>::cplx;
  const bool wh_ok = WH.expanded() && WH.cplx == cplx && !WH.slab->labelled() && (WH.rows == WH.cols || slab_panels_ok()) &&
                     (WH.zero_free == 1 || WH.slab->origin) &&   // (a view's stored zeros add nothing to the dot)
                     (!cplx || sa_readable_c(WH));
  auto ok = [](const DevMat& M) { return hpcp_operand(M, cplx); };
  if (!ok(D1) || !ok(DDH) || !ok(D2DH) || !wh_ok || &D1 == &DDH || &D1 == &D2DH || &DDH == &D2DH ||
      &OutD1 == &OutDH || D1.cols != DDH.cols || D1.cols != D2DH.cols || D1.cols != WH.cols || D1.rows != DDH.rows || D1.rows != D2DH.rows ||
      D1.rows != WH.rows || D1.slab->row_pad != DDH.slab->row_pad || D1.slab->row_pad != D2DH.slab->row_pad)
    return false;
  const SlabForm &fa = *D1.slab, &fb = *DDH.slab, &fc = *D2DH.slab;
  const int n = D1.cols, al = std::max(1, fa.row_pad);
  // (the operands' slots, and per column the diagonal's slot and the pads of a hull -- with room for diagonals away from their runs)
  const int64_t bound = fa.slots + fb.slots + fc.slots + 6LL * al * n;
  FreshSlabs fs(n, 2, bound, cplx, true);
  const SlabRuns ra = slab_runs(D1), rb = slab_runs(DDH), rc = slab_runs(D2DH);
  hipLaunchKernelGGL(k_hpcp_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), ra, rb, rc, n, col_offset, al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL((k_hpcp_update<T, KC>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, ra, rb, rc, slab_runs(WH), col_offset,
                     -1.0 * 2.0 * sigma, al, fs.base.p, fs.out(0), fs.out(1), bound, fs.part.p, fs.stat.p);
  DevMat R[2];
  double e = 0.0;
  if (!fs.finish("hpcp update", D1.rows, al, R, &e, 1)) return false;
  bump_matrix_value_epoch();   // (of the calls it replaces, the two merges into D1 are in place: slab_axpby counts them so)
  bump_matrix_value_epoch();
  OutD1 = std::move(R[0]);
  OutDH = std::move(R[1]);
  *energy = e;
  return true;
}
}  // namespace

bool slab_hpcp_traces(const DevMat& DDH, const DevMat& D2DH, int32_t col_offset, double out2[2]) {
  auto ok = [](const DevMat& M) { return M.expanded() && !M.cplx && !M.slab->labelled(); };   // (what slab_trace takes)
  if (!ok(DDH) || !ok(D2DH) || DDH.cols != D2DH.cols) return false;
  return hpcp_traces_run<double>(DDH, D2DH, col_offset, out2);
}
bool slab_hpcp_traces_c(const DevMat& DDH, const DevMat& D2DH, int32_t col_offset, double out2[2]) {
  // (what slab_dot_trace_c takes for its trace: a read-only view's stored zeros are zeros of the run)
  if (!sa_readable_c(DDH) || !sa_readable_c(D2DH) || DDH.cols != D2DH.cols) return false;
  return hpcp_traces_run<double2>(DDH, D2DH, col_offset, out2);
}

bool slab_hpcp_update(const DevMat& D1, const DevMat& DDH, const DevMat& D2DH, double sigma, const DevMat& WH, int32_t col_offset, DevMat& OutD1,
                      DevMat& OutDH, double* energy) {
  return hpcp_update_run<double, HPCP_KC>(D1, DDH, D2DH, sigma, WH, col_offset, OutD1, OutDH, energy);
}
bool slab_hpcp_update_c(const DevMat& D1, const DevMat& DDH, const DevMat& D2DH, double sigma, const DevMat& WH, int32_t col_offset, DevMat& OutD1,
                        DevMat& OutDH, double* energy) {
  return hpcp_update_run<double2, HPCP_KC_C>(D1, DDH, D2DH, sigma, WH, col_offset, OutD1, OutDH, energy);
}

// ------------------------------------------------------------------ ScaleAndFold: the update, the energy and the next trace of a step
// DensityMatrixSolversModule.F90:1049-1081 builds around its one product X2 = X X, with the vocabulary at threshold 0,
//   fold  (trace(X) <= trace):  x = (2 alpha) x;  x = x + (-alpha^2) x2;  energy = 2 dot(x, wh);  the next step begins with trace(x)
//   scale (trace(X) >  trace):  the product's result becomes X;           energy = 2 dot(x, wh);  likewise
// k_saf_update is the fold branch in one pass over the runs of X, X2 and WH; k_saf_dot_trace is what follows the product of the scale
// branch, one pass over the new X and WH.  Both leave per column the pair (sum of x wh, the new X's diagonal entry): sum_pairs_async
// sums the members of the pairs independently, so the second sum has the bits of slab_trace on the new X -- the trace steers the
// next branch -- and the first is the dot's terms in another fixed order.
namespace {
// the aligned hull of the two runs, per column (nothing where both are empty)
__global__ void k_saf_span(SlabRuns A, SlabRuns B, int n, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
  if (A.last[j] >= A.first[j]) { f = min(f, A.first[j]); l = max(l, A.last[j]); }
  if (B.last[j] >= B.first[j]) { f = min(f, B.first[j]); l = max(l, B.last[j]); }
  span[j] = l >= 0 ? (l / al + 1) * al - f / al * al : 0;
}
// chunks of 64 rows whose loads (three operands each) are all requested before the first of them is used: HPCP_KC's depth with
// three operands instead of four -- 12 loads per lane, a hull of up to 256 aligned rows is one trip
constexpr int SAF_KC = 4;
// ... and on runs of (re, im) pairs (option complex_scale_fold), one 16-byte load per lane and operand: two chunks in flight are
// the 24 VGPRs of load data the real kernel's four are; a hull of up to 128 aligned rows is one trip
constexpr int SAF_KC_C = 2;
// One wave per column, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of A = X and B = X2.  o1 = the new X into
// the slot at base[j]; sb = 2 alpha and sa = -alpha^2 as the host rounds them: s = sb x (ScaleMatrix), o = s + sa x2 (IncrementMatrix
// at threshold 0: isr_merge).  part[2 j] = sum over the column of o wh, a lane-strided sum then a wave sum (fixed shapes: the same
// value every run); part[2 j + 1] = o on the diagonal row, what k_sa_diag reads from the new X (0 where the row is absent).
// stat |= 1: a scaled entry underflows to zero; |= 2: runs far apart or a slot beyond the output buffer -- nothing is written for
// that column (k_hpcp_update).
// T = double2: the runs, the slots, base and bound count (re, im) pairs; both factors are real, so the scaling and the merge work
// part by part and keep an entry where either part is not zero; the dot's term is Re conj(o) wh (hpcp_term) and the diagonal's
// the real part, as k_sa_dot_trace_c reads them.
template <typename T, int KC>
__global__ __launch_bounds__(256) void k_saf_update(int n, SlabRuns A, SlabRuns B, SlabRuns W, int col_offset, double sa, double sb, int al,
                                                    const int64_t* __restrict__ base, IsrOut o1, int64_t bound, double* __restrict__ part,
                                                    unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = A.first[j], lA = A.last[j], fB = B.first[j], lB = B.last[j], fW = W.first[j], lW = W.last[j];
  const int dg = j + col_offset;
  const bool anyA = lA >= fA, anyB = lB >= fB, anyW = lW >= fW;
  const int64_t slot = base[j];
  int f = INT_MAX, l = -1, own = 0;   // the hull of the two runs, and the rows their own aligned slots hold
  if (anyA) { f = min(f, fA); l = max(l, lA); own += (lA / al + 1) * al - fA / al * al; }
  if (anyB) { f = min(f, fB); l = max(l, lB); own += (lB / al + 1) * al - fB / al * al; }
  const int a0 = l >= 0 ? f / al * al : 0, a1 = l >= 0 ? (l / al + 1) * al : 0;
  // (runs far apart: their hull is not bounded by the two slots and the pads between them -- refused per column)
  if (a1 - a0 > own + 2 * al || slot + (int64_t)(a1 - a0) > bound || l < 0) {
    if (lane == 0) {
      o1.first[j] = INT_MAX; o1.last[j] = -1; o1.count[j] = 0; o1.off[j] = slot;
      part[2 * (size_t)j] = 0.0; part[2 * (size_t)j + 1] = 0.0;
      if (l >= 0) atomicOr(stat, 2ull);   // (a column empty in both operands is an empty column of the result)
    }
    return;
  }
  const T *__restrict__ va0 = reinterpret_cast<const T*>(A.val), *__restrict__ vb0 = reinterpret_cast<const T*>(B.val);
  const T* __restrict__ vw0 = reinterpret_cast<const T*>(W.val);
  const T* __restrict__ pa = anyA ? va0 + (A.off[j] - fA) : va0;
  const T* __restrict__ pb = anyB ? vb0 + (B.off[j] - fB) : vb0;
  const T* __restrict__ pw = anyW ? vw0 + (W.off[j] - fW) : vw0;
  T* __restrict__ d1 = static_cast<T*>(o1.val) + (slot - a0);
  int uf = 0, c1 = 0, f1 = INT_MAX, l1 = -1;
  double e = 0.0;
  for (int rb = a0; rb < a1; rb += KC * WAVE) {
    T va[KC], vb[KC], vw[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int r = rb + k * WAVE + lane;
      va[k] = (anyA && r >= fA && r <= lA) ? pa[r] : Sc<T>::zero();
      vb[k] = (anyB && r >= fB && r <= lB) ? pb[r] : Sc<T>::zero();
      vw[k] = (anyW && r >= fW && r <= lW) ? pw[r] : Sc<T>::zero();
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int r = rb + k * WAVE + lane;
      if (r >= a1) continue;
      const T x = va[k], x2 = vb[k];
      bool ho;
      const T s = Sc<T>::scale(sb, x);                                                                  // ScaleMatrix(X, 2 alpha)
      const T o = isr_merge<T>(1.0, s, !Sc<T>::is_zero(x), sa, x2, !Sc<T>::is_zero(x2), &ho, &uf);      // IncrementMatrix(X2, X, -alpha^2)
      d1[r] = o;
      e = __dadd_rn(e, hpcp_term(o, vw[k]));                                                            // DotMatrix(X, WH)
      if (r == dg) part[2 * (size_t)j + 1] = Sc<T>::re(o);                                              // MatrixTrace(X) of the next step
      c1 += ho ? 1 : 0; f1 = min(f1, ho ? r : INT_MAX); l1 = max(l1, ho ? r : -1);
    }
  }
  c1 = (int)wave_sum_i64(c1);
  f1 = wave_min_i32(f1);
  l1 = wave_max_i32(l1);
  e = wave_sum_f64(e);
  if (__ballot(uf != 0) && lane == 0) atomicOr(stat, 1ull);
  if (lane == 0) {
    o1.first[j] = f1; o1.last[j] = l1; o1.count[j] = c1;
    o1.off[j] = slot + (c1 ? f1 - a0 : 0);
    part[2 * (size_t)j] = e;
    if (dg < a0 || dg >= a1) part[2 * (size_t)j + 1] = 0.0;   // (inside the hull the lane on the diagonal row has written it)
  }
}
// One wave per column of A = the new X: part[2 j] = sum over the rows both runs hold of x wh (lane-strided, then a wave sum),
// part[2 j + 1] = X's diagonal entry as k_sa_diag reads it.  Writes nothing else.
__global__ __launch_bounds__(256) void k_saf_dot_trace(int n, SlabRuns A, SlabRuns W, int col_offset, double* __restrict__ part) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const int fA = A.first[j], lA = A.last[j], fW = W.first[j], lW = W.last[j], dg = j + col_offset;
  const bool anyA = lA >= fA, anyW = lW >= fW;
  double e = 0.0;
  if (anyA && anyW) {
    const int lo = max(fA, fW), hi = min(lA, lW);
    const double* __restrict__ pa = A.val + (A.off[j] - fA);
    const double* __restrict__ pw = W.val + (W.off[j] - fW);
    for (int rb = lo; rb <= hi; rb += SAF_KC * WAVE) {
      double va[SAF_KC], vw[SAF_KC];
#pragma unroll
      for (int k = 0; k < SAF_KC; ++k) {
        const int r = rb + k * WAVE + lane;
        va[k] = r <= hi ? pa[r] : 0.0;
        vw[k] = r <= hi ? pw[r] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < SAF_KC; ++k) e = __dadd_rn(e, __dmul_rn(va[k], vw[k]));
    }
  }
  e = wave_sum_f64(e);
  if (lane == 0) {
    part[2 * (size_t)j] = e;
    part[2 * (size_t)j + 1] = (anyA && dg >= fA && dg <= lA) ? A.val[A.off[j] + (dg - fA)] : 0.0;
  }
}
// WH of the energy's dot: a zero-free slab form or a read-only view (a view's stored zeros add nothing to the dot)
bool saf_wh_ok(const DevMat& WH) {
  return WH.expanded() && !WH.cplx && !WH.slab->labelled() && (WH.rows == WH.cols || slab_panels_ok()) && (WH.zero_free == 1 || WH.slab->origin);
}
// the fold update on operands of one kind; the slots, `bound` and the output's buffer count entries of T
template <typename T, int KC>
bool saf_update_run(const DevMat& X, const DevMat& X2, double a, double b, const DevMat& WH, int32_t col_offset, DevMat& Out, double* dot,
                    double* trace) {
  constexpr bool cplx = Sc<T>::cplx;
  const bool wh_ok = cplx ? WH.cplx && sa_readable_c(WH) && (WH.zero_free == 1 || WH.slab->origin) : saf_wh_ok(WH);
  if (!hpcp_operand(X, cplx) || !hpcp_operand(X2, cplx) || !wh_ok || &X == &X2 || X.cols != X2.cols || X.cols != WH.cols || X.rows != X2.rows ||
      X.rows != WH.rows || X.slab->row_pad != X2.slab->row_pad || !std::isfinite(a) || !std::isfinite(b))
    return false;
  const SlabForm &fa = *X.slab, &fb = *X2.slab;
  const int n = X.cols, al = std::max(1, fa.row_pad);
  // (the operands' slots and per column the pads of a hull)
  const int64_t bound = fa.slots + fb.slots + 4LL * al * n;
  FreshSlabs fs(n, 1, bound, cplx, true);
  const SlabRuns ra = slab_runs(X), rb = slab_runs(X2);
  hipLaunchKernelGGL(k_saf_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), ra, rb, n, al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL((k_saf_update<T, KC>), dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, ra, rb, slab_runs(WH), col_offset, a, b,
                     al, fs.base.p, fs.out(0), bound, fs.part.p, fs.stat.p);
  DevMat R;
  double sums[2] = {0.0, 0.0};
  if (!fs.finish("scale and fold update", X.rows, al, &R, sums, 2)) return false;
  bump_matrix_value_epoch();   // (the merge it replaces is in place: slab_axpby counts it so)
  Out = std::move(R);
  *dot = sums[0];
  *trace = sums[1];
  return true;
}
}  // namespace

bool slab_saf_update(const DevMat& X, const DevMat& X2, double a, double b, const DevMat& WH, int32_t col_offset, DevMat& Out, double* dot,
                     double* trace) {
  return saf_update_run<double, SAF_KC>(X, X2, a, b, WH, col_offset, Out, dot, trace);
}
bool slab_saf_update_c(const DevMat& X, const DevMat& X2, double a, double b, const DevMat& WH, int32_t col_offset, DevMat& Out, double* dot,
                       double* trace) {
  return saf_update_run<double2, SAF_KC_C>(X, X2, a, b, WH, col_offset, Out, dot, trace);
}

bool slab_saf_dot_trace(const DevMat& X, const DevMat& WH, int32_t col_offset, double* dot, double* trace) {
  if (!hpcp_operand(X) || !saf_wh_ok(WH) || X.cols != WH.cols || X.rows != WH.rows) return false;
  const int n = X.cols;
  DevBuf<double> part((size_t)2 * n);
  hipLaunchKernelGGL(k_saf_dot_trace, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, slab_runs(X), slab_runs(WH), col_offset, part.p);
  double sums[2] = {0.0, 0.0};
  fetch_pair_sums(part, n, sums);
  *dot = sums[0];
  *trace = sums[1];
  return true;
}

long long slab_product_count(const DevMat& A, const DevMat& B) {
  if (!A.expanded() || !B.expanded() || A.cplx || B.cplx) return 0;
  const SlabForm &fa = *A.slab, &fb = *B.slab;
  DevBuf<unsigned long long> acc(1);
  acc.zero();
  hipLaunchKernelGGL(k_sa_products, dim3(cdiv((int64_t)B.cols * WAVE, 256)), dim3(256), 0, stream(), B.cols, fb.first.p, fb.last.p,
                     fb.off.p, fb.val.p, fa.count.p, A.cols, acc.p);
  unsigned long long h = 0;
  ScalarFetch f;
  f.add(acc.p, 1, &h);
  f.run();
  return (long long)h;
}

// ------------------------------------------------------------------ the transpose of a slab form (option slab_transpose)
// AT(j, i) = A(i, j) (conj: its conjugate) for a square, zero-free, unlabelled slab form A that is no view, as a fresh slab form
// with A's row_pad: the Polar loop's U^H and a caller's Transpose of a product without leaving the tile kernel's operand form.
// Three steps on the FreshSlabs scaffold, one host wait:
//   1. k_tr_extents: column i of AT spans the first to the last j with A(i, j) != 0 (complex: either part) and holds `count` of
//      them.  A workgroup walks TR_CB consecutive columns of A in tiles of 64 rows, lanes along rows (the runs are read
//      coalesced), every wave two of each eight columns in ascending order; the four waves' (min, max, count) per row meet in
//      LDS and ONE atomicMin / atomicMax / atomicAdd per row and column block goes out.  Integer atomics only: the same bits
//      every run.
//   2. k_tr_span: spans aligned to row_pad (an empty column: none), then the scan.
//   3. k_tr_values: a workgroup owns TR_T consecutive columns of AT and walks their aligned hull in tiles of TR_T rows: the tile
//      of A is read with lanes along A's rows into LDS (pitch TR_T + 1 elements: the transposed read then touches every bank
//      once), and written with lanes along AT's rows.  Every slot of [a0, a1) of every column is written exactly once, zeros
//      where A has no entry; a zero inside a run of A (padding, a hole) is no entry.  A slot total beyond `bound`: stat |= 2,
//      nothing written.
// No matrix instruction, no scratch.
namespace {
constexpr int TR_CB = 32;   // columns of A per workgroup of the extents pass
constexpr int TR_T = 32;    // tile edge of the values pass
__global__ void k_tr_init(int n, int32_t* __restrict__ ofirst, int32_t* __restrict__ olast, int32_t* __restrict__ ocount) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ofirst[i] = INT_MAX;
  olast[i] = -1;
  ocount[i] = 0;
}
template <typename T>
__global__ __launch_bounds__(256) void k_tr_extents(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                    const int64_t* __restrict__ offa, const T* __restrict__ va, int32_t* __restrict__ ofirst,
                                                    int32_t* __restrict__ olast, int32_t* __restrict__ ocount) {
  __shared__ int sf[TR_CB], sl[TR_CB];
  __shared__ long long so[TR_CB];
  __shared__ int rmn[4][WAVE], rmx[4][WAVE], rct[4][WAVE];
  const int c0 = blockIdx.x * TR_CB, t = threadIdx.x, lane = t % WAVE, w = t / WAVE;
  if (t < TR_CB) {
    const int j = c0 + t;
    const bool in = j < n;
    sf[t] = in ? fa[j] : INT_MAX;
    sl[t] = in ? la[j] : -1;
    so[t] = in ? offa[j] : 0;
  }
  __syncthreads();
  int lo = INT_MAX, hi = -1;
  for (int c = 0; c < TR_CB; ++c)
    if (sl[c] >= sf[c]) { lo = min(lo, sf[c]); hi = max(hi, sl[c]); }
  if (hi < lo) return;   // (uniform: every column of the block is empty)
  for (int r0 = lo / WAVE * WAVE; r0 <= hi; r0 += WAVE) {
    const int r = r0 + lane;
    int mn = INT_MAX, mx = -1, ct = 0;
    for (int q = 0; q < TR_CB / 4; ++q) {
      const int c = w * (TR_CB / 4) + q, f = sf[c], l = sl[c];
      if (r >= f && r <= l) {
        const T v = va[so[c] + (r - f)];
        if (!Sc<T>::is_zero(v)) { mn = min(mn, c0 + c); mx = max(mx, c0 + c); ct += 1; }
      }
    }
    rmn[w][lane] = mn; rmx[w][lane] = mx; rct[w][lane] = ct;
    __syncthreads();
    if (w == 0) {
      const int cnt = rct[0][lane] + rct[1][lane] + rct[2][lane] + rct[3][lane];
      if (cnt > 0 && r < n) {
        atomicMin(&ofirst[r], min(min(rmn[0][lane], rmn[1][lane]), min(rmn[2][lane], rmn[3][lane])));
        atomicMax(&olast[r], max(max(rmx[0][lane], rmx[1][lane]), max(rmx[2][lane], rmx[3][lane])));
        atomicAdd(&ocount[r], cnt);
      }
    }
    __syncthreads();
  }
}
__global__ void k_tr_span(const int32_t* __restrict__ ofirst, const int32_t* __restrict__ olast, int n, int al, int32_t* __restrict__ span) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = ofirst[i], l = olast[i];
  span[i] = l >= f ? (l / al + 1) * al - f / al * al : 0;
}
template <typename T>
__global__ __launch_bounds__(256) void k_tr_values(int n, const int32_t* __restrict__ fa, const int32_t* __restrict__ la,
                                                   const int64_t* __restrict__ offa, const T* __restrict__ va, int conj, int al,
                                                   const int64_t* __restrict__ base, const int32_t* __restrict__ ofirst,
                                                   const int32_t* __restrict__ olast, int64_t* __restrict__ ooff, T* __restrict__ out,
                                                   int64_t bound, unsigned long long* __restrict__ stat) {
  __shared__ T tile[TR_T][TR_T + 1];
  __shared__ int sa0[TR_T], sa1[TR_T];       // the aligned extent [a0, a1) of AT's columns i0 .. (empty: a1 = a0 = 0)
  __shared__ long long sbase[TR_T];
  __shared__ int sf[TR_T], sl[TR_T];         // the runs of A's columns of the current tile
  __shared__ long long so[TR_T];
  const int t = threadIdx.x, i0 = blockIdx.x * TR_T;
  if (base[n] > bound) {   // (runs far apart: the transposed extents do not fit the output -- refused by the host)
    if (blockIdx.x == 0 && t == 0) atomicOr(stat, 2ull);
    return;
  }
  if (t < TR_T) {
    const int i = i0 + t;
    int a0 = 0, a1 = 0;
    long long b = 0;
    if (i < n) {
      const int f = ofirst[i], l = olast[i];
      b = base[i];
      if (l >= f) { a0 = f / al * al; a1 = (l / al + 1) * al; }
      ooff[i] = b + (l >= f ? f - a0 : 0);
    }
    sa0[t] = a0; sa1[t] = a1; sbase[t] = b;
  }
  __syncthreads();
  int lo = INT_MAX, hi = -1;
  for (int c = 0; c < TR_T; ++c)
    if (sa1[c] > sa0[c]) { lo = min(lo, sa0[c]); hi = max(hi, sa1[c]); }
  if (hi < lo) return;   // (uniform: every column of the block is empty)
  const int lx = t % TR_T, ly = t / TR_T;   // (256 threads: 8 rows of the tile per sweep)
  for (int j0 = lo / TR_T * TR_T; j0 < hi; j0 += TR_T) {
    if (t < TR_T) {
      const int j = j0 + t;
      const bool in = j < n;
      sf[t] = in ? fa[j] : INT_MAX;
      sl[t] = in ? la[j] : -1;
      so[t] = in ? offa[j] : 0;
    }
    __syncthreads();
    // A(i0 + lx, j0 + c): lanes along the rows of A
    for (int c = ly; c < TR_T; c += 256 / TR_T) {
      const int r = i0 + lx, f = sf[c], l = sl[c];
      T v = Sc<T>::zero();
      if (r >= f && r <= l) v = va[so[c] + (r - f)];
      tile[c][lx] = (conj && !Sc<T>::is_zero(v)) ? Sc<T>::conj(v) : v;   // (k_conj's negation; a slot without an entry stays (0, 0))
    }
    __syncthreads();
    // AT(j0 + lx, i0 + c): lanes along the rows of AT
    for (int c = ly; c < TR_T; c += 256 / TR_T) {
      const int j = j0 + lx, a0 = sa0[c];
      if (j >= a0 && j < sa1[c]) out[sbase[c] + (j - a0)] = tile[lx][c];
    }
    __syncthreads();
  }
}
}  // namespace

bool slab_transpose_operand(const DevMat& A) {
  return A.expanded() && A.rows == A.cols && !A.slab->labelled() && !A.slab->origin && A.zero_free == 1 && !slab_panels_ok() &&
         (A.cplx ? A.slab->row_pad % 16 == 0 : (A.slab->row_pad == 1 || A.slab->row_pad % 16 == 0));
}

template <typename T>
bool slab_transpose(const DevMat& A, bool conj, DevMat& AT) {
  if (!slab_transpose_operand(A) || A.cplx != Sc<T>::cplx) return false;
  const SlabForm& fa = *A.slab;
  const int n = A.cols, al = std::max(1, fa.row_pad);
  const int64_t bound = 4 * fa.slots + 4LL * al * n;   // (slots of T)
  FreshSlabs fs(n, 1, bound, Sc<T>::cplx, false);
  const IsrOut o = fs.out(0);
  const T* va = reinterpret_cast<const T*>(fa.val.p);
  // (statistics, option time_kernels with NTPOLY_AMD_DEBUG_SPGEMM set: the pass between two events, for tools/bench_polar_session.py)
  const bool timed = options().time_kernels != 0 && std::getenv("NTPOLY_AMD_DEBUG_SPGEMM") != nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (timed) {
    HIP_CHECK(hipEventCreate(&ev[0]));
    HIP_CHECK(hipEventCreate(&ev[1]));
    HIP_CHECK(hipEventRecord(ev[0], stream()));
  }
  hipLaunchKernelGGL(k_tr_init, dim3(cdiv(n, 256)), dim3(256), 0, stream(), n, o.first, o.last, o.count);
  hipLaunchKernelGGL((k_tr_extents<T>), dim3(cdiv(n, TR_CB)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p, va, o.first, o.last, o.count);
  hipLaunchKernelGGL(k_tr_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), o.first, o.last, n, al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL((k_tr_values<T>), dim3(cdiv(n, TR_T)), dim3(256), 0, stream(), n, fa.first.p, fa.last.p, fa.off.p, va, conj ? 1 : 0, al,
                     fs.base.p, o.first, o.last, o.off, static_cast<T*>(o.val), bound, fs.stat.p);
  if (timed) HIP_CHECK(hipEventRecord(ev[1], stream()));
  DevMat R;
  const bool done = fs.finish("slab transpose", A.rows, al, &R);
  if (timed) {   // (finish waited for the stream)
    float ms = 0.f;
    HIP_CHECK(hipEventSynchronize(ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    HIP_CHECK(hipEventDestroy(ev[0]));
    HIP_CHECK(hipEventDestroy(ev[1]));
    // bytes: the runs of A read by the extents pass and by the values pass, the runs of AT written, the extents of both
    const double bytes = (double)sizeof(T) * (2.0 * (double)fa.slots + (done ? (double)R.slab->slots : 0.0)) + 40.0 * (double)n;
    std::fprintf(stderr, "[slab transpose] timed: n %d slots_in %lld slots_out %lld bytes %.0f ms %.5f\n", n, (long long)fa.slots,
                 done ? (long long)R.slab->slots : -1LL, bytes, (double)ms);
  }
  if (!done) return false;
  AT = std::move(R);
  return true;
}
template bool slab_transpose<double>(const DevMat& A, bool conj, DevMat& AT);
template bool slab_transpose<double2>(const DevMat& A, bool conj, DevMat& AT);

bool slab_transpose_any(const DevMat& A, bool conj, DevMat& AT) {
  return A.cplx ? slab_transpose<double2>(A, conj, AT) : slab_transpose<double>(A, conj, AT);
}

// ConjugateMatrix of a complex slab form in place: one pass over the runs, k_conj's negation on every entry (pads and holes stay
// (0, 0)); the moduli, and with them amax, stay what they were
namespace {
__global__ __launch_bounds__(256) void k_sa_conj(int n, const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                 const int64_t* __restrict__ off, double2* __restrict__ val) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int f = first[j], l = last[j];
  if (l < f) return;
  double2* __restrict__ v = val + off[j];
  for (int r = lane_id(); r <= l - f; r += WAVE) {
    const double2 e = v[r];
    if (!Sc<double2>::is_zero(e)) v[r].y = -e.y;
  }
}
}  // namespace
bool slab_conjugate_c(DevMat& A) {
  if (!sa_operand_c(A) || A.zero_free != 1) return false;
  SlabForm& f = *A.slab;
  bump_matrix_value_epoch();
  hipLaunchKernelGGL(k_sa_conj, dim3(cdiv((int64_t)A.cols * WAVE, 256)), dim3(256), 0, stream(), A.cols, f.first.p, f.last.p, f.off.p,
                     reinterpret_cast<double2*>(f.val.p));
  f.tiles.release();   // (multiplier tiles would hold the old values)
  f.tile_off.release();
  return true;
}

}  // namespace ntp
