// The input and sweep scaffold of the fused slab merge passes (pade_chain.hip, sum_chain.hip, poly_step.hip, purify_tail.hip,
// wom_heun.hip; the runs struct also in slab_extra.hip and cg_dots.hip), as fresh_slabs.hpp is their output scaffold: an operand's
// runs, one column of them, the span kernel over the aligned hull of K operands' runs, the hull and kept extent of a column, the
// threshold-0 merge step, and hull_sweep(): one wave per column over that hull.  A new pass of this kind writes a row functor (the
// arithmetic of one row) and a host frame (which operands, which alignment, which bound).  Everything sits in an anonymous namespace.
// NOT for the threshold-aware merges of slab_extra.hip (PmRuns / PmCol, isr_merge, pm_merge, step_merge, k_sa_recurrence_step_c):
// they look at the other operand's last row and carry two slots per column -- another rule set.
//
// Every merge here is AddSparseVectors at threshold 0 as k_sa_axpby (kernels.hip) restates it on runs: the scaled addend is rounded,
// then added; a row both operands hold is kept iff the sum is not zero -- a row that cancels is ABSENT for the next addend; a row one
// operand holds keeps its (non-zero) value.  At threshold 0, on zero-free operands, no rule looks at the other operand's last row,
// so ONE sweep decides a column.
//
// stat |= 1: a scaled value is exactly zero where an entry is held (compressed columns would store it, no run can); |= 2: runs far
// apart (the hull is not bounded by the inputs' own slots and pads), a slot beyond the output buffer, or an input that is not
// finite -- the pass is refused.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "fresh_slabs.hpp"

namespace ntp {
namespace {
struct SlabRuns {   // one operand in slab form
  const int32_t* first;
  const int32_t* last;
  const int64_t* off;
  const double* val;
};
SlabRuns slab_runs(const DevMat& M) { return SlabRuns{M.slab->first.p, M.slab->last.p, M.slab->off.p, M.slab->val.p}; }

template <typename T>
struct SlabCol {   // one column of an operand: p[r] is row r for f <= r <= l (an empty column: f = INT_MAX, l = -1)
  const T* p;
  int f, l;
};
template <typename T>
__device__ inline SlabCol<T> slab_col(const SlabRuns& R, int j) {
  const int f = R.first[j], l = R.last[j];
  const T* v = reinterpret_cast<const T*>(R.val);
  if (l < f) return SlabCol<T>{v, INT_MAX, -1};
  return SlabCol<T>{v + (R.off[j] - f), f, l};
}
template <typename T>
__device__ inline T slab_at(const SlabCol<T>& c, int r) { return (r >= c.f && r <= c.l) ? c.p[r] : Sc<T>::zero(); }
__device__ inline bool slab_finite(double v) { return isfinite(v); }
__device__ inline bool slab_finite(double2 v) { return isfinite(v.x) && isfinite(v.y); }

template <int K>
struct SlabIn {   // the K operands whose runs a pass merges
  SlabRuns in[K];
};
// the aligned hull of the runs of all K operands, per column (nothing where all are empty): the slot of the pass's outputs
template <int K>
__global__ void k_hull_span(SlabIn<K> P, int n, int al, int32_t* __restrict__ span) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int f = INT_MAX, l = -1;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (P.in[k].last[j] >= P.in[k].first[j]) { f = min(f, P.in[k].first[j]); l = max(l, P.in[k].last[j]); }
  span[j] = l >= 0 ? (l / al + 1) * al - f / al * al : 0;
}

// the hull [f, l] of K columns' runs (l < 0: all empty), the rows `own` that their own aligned slots hold, and the aligned hull
// [a0, a1).  apart(): the hull is not bounded by the K slots and the pads between them -- the column is refused
struct SlabHull {
  int f = INT_MAX, l = -1, own = 0, a0 = 0, a1 = 0;
  template <typename T, int K>
  __device__ inline SlabHull(const SlabCol<T> (&col)[K], int al) {
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (col[k].l >= 0) { f = min(f, col[k].f); l = max(l, col[k].l); own += (col[k].l / al + 1) * al - col[k].f / al * al; }
    if (l >= 0) { a0 = f / al * al; a1 = (l / al + 1) * al; }
  }
  __device__ inline bool apart(int K, int al) const { return a1 - a0 > own + K * al; }
};
__device__ inline void slab_empty_column(const IsrOut& o, int j, int64_t slot) {
  o.first[j] = INT_MAX; o.last[j] = -1; o.count[j] = 0; o.off[j] = slot;
}
// the kept rows of one output column: per lane, then reduce() over the wave, then store() by one lane
struct KeptExtent {
  int cnt = 0, kf = INT_MAX, kl = -1;
  __device__ inline void note(bool has, int r) {
    cnt += has ? 1 : 0;
    kf = min(kf, has ? r : INT_MAX);
    kl = max(kl, has ? r : -1);
  }
  __device__ inline void reduce() {
    cnt = (int)wave_sum_i64(cnt);
    kf = wave_min_i32(kf);
    kl = wave_max_i32(kl);
  }
  __device__ inline void store(const IsrOut& o, int j, int64_t slot, int a0) const {
    o.first[j] = kf; o.last[j] = kl; o.count[j] = cnt;
    o.off[j] = slot + (cnt ? kf - a0 : 0);
  }
};

// one row of IncrementMatrix(A, B, c, 0): wa = the scaled addend (held iff ha), v the running value (held iff has); alone() runs
// where the addend alone holds the row
template <typename T, typename Alone>
__device__ inline void merge0(T wa, bool ha, T& v, bool& has, const Alone& alone) {
  if (ha && has) { v = Sc<T>::add(wa, v); has = !Sc<T>::is_zero(v); }
  else if (ha) { v = wa; has = true; alone(); }
}
template <typename T>
__device__ inline void merge0(T wa, bool ha, T& v, bool& has) { merge0(wa, ha, v, has, [] {}); }

// One wave per column j, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of the K operands, chunks of 64 rows
// whose K loads are all requested before the first of them is used.  row(x, emit, zk): from the K values x of a row it calls
// emit(q, v, has) once per output q (v zero where has is false) and ORs the stored-zero flag into zk.  Output q goes into the slot
// at base[j] of o[q] (every row of the hull written: pads and dropped rows zero) with its own extent and count; the outputs may end
// with different patterns in the same slots.  Runs far apart are refused per column; a column empty in every input is an empty
// column of every output.
template <typename T, int K, int OUTS, typename Row>
__device__ inline void hull_sweep(int j, int lane, const SlabIn<K>& P, const Row& row, int al, const int64_t* __restrict__ base,
                                  const IsrOut (&o)[OUTS], int64_t bound, unsigned long long* __restrict__ stat) {
  SlabCol<T> col[K];
#pragma unroll
  for (int k = 0; k < K; ++k) col[k] = slab_col<T>(P.in[k], j);
  const SlabHull h(col, al);
  const int64_t slot = base[j];
  const int a0 = h.a0, a1 = h.a1;
  if (h.l < 0 || h.apart(K, al) || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < OUTS; ++q) slab_empty_column(o[q], j, slot);
      if (h.l >= 0) atomicOr(stat, 2ull);
    }
    return;
  }
  T* __restrict__ d[OUTS];
#pragma unroll
  for (int q = 0; q < OUTS; ++q) d[q] = static_cast<T*>(o[q].val) + (slot - a0);
  int zk = 0, bad = 0;
  KeptExtent kept[OUTS];
  for (int r = a0 + lane; r < a1; r += WAVE) {
    T x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = slab_at(col[k], r);
    row(x, [&](int q, T v, bool has) { d[q][r] = v; kept[q].note(has, r); }, zk);
#pragma unroll
    for (int k = 0; k < K; ++k) bad |= slab_finite(x[k]) ? 0 : 1;
  }
#pragma unroll
  for (int q = 0; q < OUTS; ++q) kept[q].reduce();
  const bool anyz = __ballot(zk != 0) != 0, anyb = __ballot(bad != 0) != 0;
  if (lane == 0) {
    if (anyz) atomicOr(stat, 1ull);
    if (anyb) atomicOr(stat, 2ull);
#pragma unroll
    for (int q = 0; q < OUTS; ++q) kept[q].store(o[q], j, slot, a0);
  }
}

// ------------------------------------------------------------------ the host frame of a pass
// what a pass merges: an unlabelled, zero-free slab form of the pass's kind (real or complex) that is no view (square, or a column
// panel in a panel session)
bool slab_merge_operand(const DevMat& M, bool cplx) {
  return M.expanded() && M.cplx == cplx && (M.rows == M.cols || slab_panels_ok()) && !M.slab->labelled() && !M.slab->origin && M.zero_free == 1;
}
// (ScaleMatrix by zero and a zero coefficient leave stored zeros, a scalar that is not finite nothing a run can hold)
bool scalar_usable(double s) { return std::isfinite(s) && s != 0.0; }
// K distinct operands of one shape and, with same_pad, one alignment
bool same_frame(const DevMat* const* in, int K, bool same_pad) {
  for (int k = 0; k < K; ++k) {
    if (in[k]->cols != in[0]->cols || in[k]->rows != in[0]->rows || (same_pad && in[k]->slab->row_pad != in[0]->slab->row_pad)) return false;
    for (int m = 0; m < k; ++m)
      if (in[m] == in[k]) return false;
  }
  return true;
}
// the runs of K operands; returns the sum of their slots (what a bound on the outputs' slots starts from)
template <int K>
int64_t slab_in(const DevMat* const* in, SlabIn<K>& I) {
  int64_t slots = 0;
  for (int k = 0; k < K; ++k) {
    I.in[k] = slab_runs(*in[k]);
    slots += in[k]->slab->slots;
  }
  return slots;
}
// the slots of a pass's outputs: the spans of the K operands' hulls, scanned into fs.base
template <int K>
void hull_slots(const SlabIn<K>& I, int n, int al, FreshSlabs& fs) {
  hipLaunchKernelGGL(k_hull_span<K>, dim3(cdiv(n, 256)), dim3(256), 0, stream(), I, n, al, fs.span.p);
  fs.scan();
}
// what stat bits 1 and 2 mean to the chain passes (the debug line)
const char* const SLAB_WHY_ZERO = " a scaled value is exactly zero where an entry is held";   // (complex: both parts)
const char* const SLAB_WHY_APART = " runs far apart or an input that is not finite";
}  // namespace
}  // namespace ntp
