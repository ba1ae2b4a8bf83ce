// The tail of a step of the Chebyshev / Hermite recurrences (ChebyshevSolversModule.F90:69-160, HermiteSolversModule.F90:52-184)
// on real slab-form matrices.  Behind the product P = 2 X T(k-1) a step makes, with the vocabulary at threshold 0,
//   IncrementMatrix(Q, P, a, 0)    Tk = P + a Q       (Q = T(k-2), a = -1)
//   IncrementMatrix(Tk, R, c, 0)   R' = R + c Tk      (R the running sum)
// -- six matrix-sized streams and two read-backs.  k_poly_step reads the runs of P, Q and R once and writes Tk and R': five streams
// and one read-back, and Tk goes from the first merge into the second in a register.
//
// Every merge is AddSparseVectors at threshold 0 as k_sa_axpby (kernels.hip) restates it on runs: the scaled addend is rounded,
// then added; a row both operands hold is kept iff the sum is not zero -- a row that cancels in the first merge is ABSENT for the
// second; a row one operand holds keeps its (non-zero) value.  At threshold 0, on zero-free operands, no rule looks at the other
// operand's last row (pade_chain.hip gives the argument), so ONE sweep decides a column and a lane needs nothing but its own row of
// Tk.  The two outputs may end with different patterns in the same slots.
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
struct PlRuns {   // one operand in slab form
  const int32_t* first;
  const int32_t* last;
  const int64_t* off;
  const double* val;
};
PlRuns pl_runs(const DevMat& M) { return PlRuns{M.slab->first.p, M.slab->last.p, M.slab->off.p, M.slab->val.p}; }
struct PlIn {   // in[0] = P, in[1] = Q, in[2] = R
  PlRuns in[3];
  double a, c;
};

struct PlCol {   // one column of an operand: p[r] is row r for f <= r <= l (an empty column: f = INT_MAX, l = -1)
  const double* p;
  int f, l;
};
__device__ inline PlCol pl_col(const PlRuns& R, int j) {
  const int f = R.first[j], l = R.last[j];
  if (l < f) return PlCol{R.val, INT_MAX, -1};
  return PlCol{R.val + (R.off[j] - f), f, l};
}
__device__ inline double pl_at(const PlCol& c, int r) { return (r >= c.f && r <= c.l) ? c.p[r] : 0.0; }

// the aligned hull of the three runs, per column (nothing where all are empty): the slot of both outputs
__global__ void k_poly_span(PlIn P, int n, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (P.in[k].last[j] >= P.in[k].first[j]) { f = min(f, P.in[k].first[j]); l = max(l, P.in[k].last[j]); }
  span[j] = l >= 0 ? (l / al + 1) * al - f / al * al : 0;
}

// One wave per column, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of P, Q and R, chunks of 64 rows whose
// three loads are all requested before the first of them is used.  Tk into the slot at base[j] of ot, R' into that of orr (every
// row of the hull written: pads and dropped rows zero), each with its own extent and count.
__global__ __launch_bounds__(256) void k_poly_step(int n, PlIn P, int al, const int64_t* __restrict__ base, IsrOut ot, IsrOut orr, int64_t bound,
                                                   unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  PlCol col[3];
  int f = INT_MAX, l = -1, own = 0;   // the hull of the runs, and the rows their own aligned slots hold
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    col[k] = pl_col(P.in[k], j);
    if (col[k].l >= 0) { f = min(f, col[k].f); l = max(l, col[k].l); own += (col[k].l / al + 1) * al - col[k].f / al * al; }
  }
  const int64_t slot = base[j];
  const int a0 = l >= 0 ? f / al * al : 0, a1 = l >= 0 ? (l / al + 1) * al : 0;
  // (runs far apart: their hull is not bounded by the inputs' slots and the pads between them -- refused per column; a column
  // empty in every input is an empty column of both results)
  if (l < 0 || a1 - a0 > own + 3 * al || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
      ot.first[j] = INT_MAX; ot.last[j] = -1; ot.count[j] = 0; ot.off[j] = slot;
      orr.first[j] = INT_MAX; orr.last[j] = -1; orr.count[j] = 0; orr.off[j] = slot;
      if (l >= 0) atomicOr(stat, 2ull);
    }
    return;
  }
  double* __restrict__ dt = static_cast<double*>(ot.val) + (slot - a0);
  double* __restrict__ dr = static_cast<double*>(orr.val) + (slot - a0);
  int zk = 0, bad = 0;
  int cnt[2] = {0, 0}, kf[2] = {INT_MAX, INT_MAX}, kl[2] = {-1, -1};
  for (int r = a0 + lane; r < a1; r += WAVE) {
    const double p = pl_at(col[0], r), q = pl_at(col[1], r), s = pl_at(col[2], r);
    const bool hp = p != 0.0, hq = q != 0.0, hs = s != 0.0;
    // IncrementMatrix(Q, P, a, 0): Q the addend, P the running value
    const double wq = __dmul_rn(P.a, q);
    zk |= (hq && wq == 0.0) ? 1 : 0;
    double t = p;
    bool ht = hp;
    if (hq && hp) { t = __dadd_rn(wq, p); ht = t != 0.0; }
    else if (hq) { t = wq; ht = true; }
    t = ht ? t : 0.0;
    // IncrementMatrix(Tk, R, c, 0): Tk the addend, from the register; R the running value
    const double wt = __dmul_rn(P.c, t);
    zk |= (ht && wt == 0.0) ? 1 : 0;
    double v = s;
    bool hv = hs;
    if (ht && hs) { v = __dadd_rn(wt, s); hv = v != 0.0; }
    else if (ht) { v = wt; hv = true; }
    v = hv ? v : 0.0;
    dt[r] = t;
    dr[r] = v;
    cnt[0] += ht ? 1 : 0;
    kf[0] = min(kf[0], ht ? r : INT_MAX);
    kl[0] = max(kl[0], ht ? r : -1);
    cnt[1] += hv ? 1 : 0;
    kf[1] = min(kf[1], hv ? r : INT_MAX);
    kl[1] = max(kl[1], hv ? r : -1);
    bad |= (isfinite(p) && isfinite(q) && isfinite(s)) ? 0 : 1;
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
    ot.first[j] = kf[0]; ot.last[j] = kl[0]; ot.count[j] = cnt[0];
    ot.off[j] = slot + (cnt[0] ? kf[0] - a0 : 0);
    orr.first[j] = kf[1]; orr.last[j] = kl[1]; orr.count[j] = cnt[1];
    orr.off[j] = slot + (cnt[1] ? kf[1] - a0 : 0);
  }
}

// what the pass merges: a real, unlabelled, zero-free slab form that is no view (square, or a column panel in a panel session)
bool pl_operand(const DevMat& M) {
  return M.expanded() && !M.cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1;
}
}  // namespace

bool slab_poly_step(const DevMat& P, const DevMat& Q, const DevMat& R, double a, double c, DevMat& Tk, DevMat& Rout) {
  const DevMat* in[3] = {&P, &Q, &R};
  int al = 1;
  for (int k = 0; k < 3; ++k) {
    if (!pl_operand(*in[k]) || in[k]->cols != P.cols || in[k]->rows != P.rows) return false;
    for (int m = 0; m < k; ++m)
      if (in[m] == in[k]) return false;
    al = std::max(al, in[k]->slab->row_pad);
  }
  // (the outputs' slots are aligned to the widest alignment of the inputs, which has to hold every input's own)
  for (int k = 0; k < 3; ++k)
    if (al % std::max(1, in[k]->slab->row_pad) != 0) return false;
  if (P.cols == 0) return false;
  // (a zero coefficient leaves stored zeros, a scalar that is not finite nothing a run can hold)
  if (!std::isfinite(a) || a == 0.0 || !std::isfinite(c) || c == 0.0) return false;
  const int n = P.cols;
  PlIn I;
  int64_t slots = 0;
  for (int k = 0; k < 3; ++k) {
    I.in[k] = pl_runs(*in[k]);
    slots += in[k]->slab->slots;
  }
  I.a = a;
  I.c = c;
  // (the operands' slots, re-aligned to al, and per column the pads of a hull: what the kernel's per-column rule admits)
  const int64_t bound = slots + 9LL * al * n;
  FreshSlabs fs(n, 2, bound, false, false);
  fs.why[0] = " a scaled value is exactly zero where an entry is held";
  fs.why[1] = " runs far apart or an input that is not finite";
  hipLaunchKernelGGL(k_poly_span, dim3(cdiv(n, 256)), dim3(256), 0, stream(), I, n, al, fs.span.p);
  fs.scan();
  hipLaunchKernelGGL(k_poly_step, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, I, al, fs.base.p, fs.out(0), fs.out(1), bound, fs.stat.p);
  DevMat O[2];
  if (!fs.finish("poly step", P.rows, al, O)) return false;
  Tk = std::move(O[0]);
  Rout = std::move(O[1]);
  return true;
}

}  // namespace ntp
