// The tail of an iteration of PurificationExtrapolate (GeometryOptimizationModule.F90:24-136) on slab-form matrices.  Behind its
// two products T = D S and N = T D the loop calls, with the vocabulary at threshold 0,
//   fold  (trace > dot(D, S)):  ScaleMatrix(N, -1);  IncrementMatrix(D, N, 2)                       N' = 2 D - D S D
//   plain (otherwise):          nothing                                                              N' = D S D, the product's output
//   IncrementMatrix(N', D, -1);  norm = MatrixNorm(D);  CopyMatrix(N', D);  the next iteration begins with DotMatrix(D, S)
// -- about nine reads and four writes of runs the size of the iterate and two host read-backs.  k_purify_tail reads the runs of D, N
// and S once, writes N' in the fold branch (nothing in the plain one) and leaves per column the sum of |D - N'| and the terms of
// dot(N', S): one read-back.
//
// The rules of a merge (merge0) and the pieces of the sweep are in slab_columns.hpp.
//
// The norm ends the loop and the dot decides the next branch, so both carry the bits the session's calls give on slab-form
// matrices.  slab_norm (k_sa_colstat) gives lane t the rows first_kept + t + 64 m of the difference in ascending order, then runs
// the wave butterfly; slab_dot (k_sa_dot) gives lane t the rows f + t + 64 m from f = the later first row of N' and S.  A lane of
// the sweep holds the rows of its own residue from the hull's first row a0 -- the same rows in the same order, dropped and absent
// rows adding an exact zero -- so the 64 partial sums rotated by (first_kept - a0) & 63, resp. (f - a0) & 63, go through the same
// butterfly (sweep 3 of k_wom_heun).  The per-column pairs (dot, 0) are then summed by slab_dot's two-level sum.
//
// stat |= 1: a kept value is exactly zero (compressed columns would store it, no run can); |= 2: runs far apart (the hull of D and
// N is not bounded by their slots), a slot beyond the output buffer, or an input that is not finite -- the pass is refused.
#include <hip/hip_runtime.h>

#include "slab_columns.hpp"

namespace ntp {
namespace {
// chunks of 64 rows whose loads (three operands each) are all requested before the first of them is used, as k_saf_update: 12
// loads per lane, a hull of up to 256 aligned rows is one trip
constexpr int PT_KC = 4;

// One wave per column, lanes on consecutive rows of the aligned hull [a0, a1) of the runs of D and N.  FOLD: N' = 2 D - N into the
// slot at base[j] (every row of the hull written: pads and dropped rows zero) with its extent and count; otherwise N' = N and
// nothing is written.  colsum[j] = the column sum of |D - N'| in k_sa_colstat's order; part[2 j] = the column's share of dot(N', S)
// in k_sa_dot's order, part[2 j + 1] = 0.
template <bool FOLD>
__global__ __launch_bounds__(256) void k_purify_tail(int n, SlabRuns D, SlabRuns N, SlabRuns S, int al, const int64_t* __restrict__ base, IsrOut o1,
                                                     int64_t bound, double* __restrict__ colsum, double* __restrict__ part,
                                                     unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const SlabCol<double> dn[2] = {slab_col<double>(D, j), slab_col<double>(N, j)}, cs = slab_col<double>(S, j);
  const SlabCol<double>&cd = dn[0], &cn = dn[1];
  const int64_t slot = FOLD ? base[j] : 0;
  const SlabHull h(dn, al);   // (of D and N: S is read, it adds no row)
  const int a0 = h.a0, a1 = h.a1;
  // (runs far apart: their hull is not bounded by the two slots and the pads between them -- refused per column; a column empty
  // in both operands is an empty column of the result, a zero of the norm and of the dot)
  if (h.l < 0 || h.apart(2, al) || (FOLD && slot + (int64_t)(a1 - a0) > bound)) {
    if (lane == 0) {
      if (FOLD) slab_empty_column(o1, j, slot);
      colsum[j] = 0.0;
      part[2 * (size_t)j] = 0.0; part[2 * (size_t)j + 1] = 0.0;
      if (h.l >= 0) atomicOr(stat, 2ull);
    }
    return;
  }
  double* __restrict__ dst = FOLD ? static_cast<double*>(o1.val) + (slot - a0) : nullptr;
  int zk = 0, bad = 0, df = INT_MAX;
  KeptExtent kept;
  double pn = 0.0, pd = 0.0;   // this lane's residue of the norm's and the dot's sums, rows ascending
  for (int rb = a0; rb < a1; rb += PT_KC * WAVE) {
    double vd[PT_KC], vn[PT_KC], vs[PT_KC];
#pragma unroll
    for (int k = 0; k < PT_KC; ++k) {
      const int r = rb + k * WAVE + lane;
      vd[k] = slab_at(cd, r); vn[k] = slab_at(cn, r); vs[k] = slab_at(cs, r);
    }
#pragma unroll
    for (int k = 0; k < PT_KC; ++k) {
      const int r = rb + k * WAVE + lane;
      if (r >= a1) continue;
      const double d = vd[k], nn = vn[k], s = vs[k];
      bad |= (isfinite(d) && isfinite(nn) && isfinite(s)) ? 0 : 1;
      const bool hd = d != 0.0;
      double np = nn;   // N' on this row, 0.0 where it holds no entry
      if (FOLD) {
        // ScaleMatrix(N, -1) is exact; IncrementMatrix(D, N, 2): A = D, B = -N
        double o = -nn;
        bool keep = nn != 0.0;
        merge0(__dmul_rn(2.0, d), hd, o, keep);
        zk |= (keep && o == 0.0) ? 1 : 0;
        np = keep ? o : 0.0;
        dst[r] = np;
        kept.note(keep, r);
      }
      // IncrementMatrix(N', D, -1): A = N', B = D
      const bool hp = np != 0.0;
      const double wp = __dmul_rn(-1.0, np);
      double v = 0.0;
      if (hp && hd) v = __dadd_rn(wp, d);
      else if (hp) v = wp;
      else if (hd) v = d;
      pn = __dadd_rn(pn, fabs(v));
      df = min(df, v != 0.0 ? r : INT_MAX);
      pd = __dadd_rn(pd, __dmul_rn(np, s));   // DotMatrix(N', S)
    }
  }
  if (FOLD) {
    kept.reduce();
  } else {   // (N' is N: its extent is the run's own)
    kept.kf = cn.f;
    kept.kl = cn.l;
  }
  df = wave_min_i32(df);
  // (lane t of k_sa_colstat holds the rows first_kept + t + 64 m: the partial sum of lane (first_kept - a0 + t) & 63 here.  The
  // butterfly joins lanes t and t ^ o, the residues mod 2 o, so a cyclic shift of the lanes only swaps the operands of commutative
  // additions: the rotation restates the lane order to the letter, the bits do not depend on it)
  const int rotn = df == INT_MAX ? 0 : ((df - a0) & (WAVE - 1));
  pn = wave_sum_f64(__shfl(pn, (lane + rotn) & (WAVE - 1), WAVE));
  // (lane t of k_sa_dot holds the rows f + t + 64 m from the later first row of N' and S up to the earlier last row; the rows
  // outside add exact zeros here; runs that do not overlap: every term is zero)
  const int fdot = max(kept.kf, cs.f), ldot = min(kept.kl, cs.l);
  const int rotd = ldot >= fdot ? ((fdot - a0) & (WAVE - 1)) : 0;
  pd = wave_sum_f64(__shfl(pd, (lane + rotd) & (WAVE - 1), WAVE));
  const bool anyz = __ballot(zk != 0) != 0, anyb = __ballot(bad != 0) != 0;
  if (lane == 0) {
    if (anyz) atomicOr(stat, 1ull);
    if (anyb) atomicOr(stat, 2ull);
    if (FOLD) kept.store(o1, j, slot, a0);
    colsum[j] = pn;
    part[2 * (size_t)j] = pd; part[2 * (size_t)j + 1] = 0.0;
  }
}

// S of the dot: a zero-free slab form or a read-only view (a view's stored zeros add nothing to the dot)
bool pt_readable(const DevMat& S) {
  return S.expanded() && !S.cplx && !S.slab->labelled() && (S.rows == S.cols || slab_panels_ok()) && (S.zero_free == 1 || S.slab->origin);
}
// what the kernel's stat bits 1 and 2 mean (the debug line of either branch)
const char* const PT_WHY[2] = {" a kept value is exactly zero", SLAB_WHY_APART};
void pt_report(unsigned long long hs) {
  if (std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
    std::fprintf(stderr, "[purify tail] refused:%s%s\n", (hs & 1ull) ? PT_WHY[0] : "", (hs & 2ull) ? PT_WHY[1] : "");
}
}  // namespace

bool slab_purify_tail(const DevMat& D, const DevMat& N, const DevMat& S, bool fold, DevMat& Out, double* norm, double dot[2]) {
  const DevMat* in[3] = {&D, &N, &S};
  if (!slab_merge_operand(D, false) || !slab_merge_operand(N, false) || !pt_readable(S) || !same_frame(in, 3, false) || D.cols == 0) return false;
  const SlabForm &fd = *D.slab, &fn = *N.slab;
  if (fd.row_pad != fn.row_pad) return false;
  const int n = D.cols, al = std::max(1, fd.row_pad);
  const dim3 grid(cdiv((int64_t)n * WAVE, 256));
  const SlabRuns rd = slab_runs(D), rn = slab_runs(N), rs = slab_runs(S);
  DevBuf<double> colsum((size_t)n), part((size_t)2 * n), res(4);
  double hr[4] = {0.0, 0.0, 0.0, 0.0};
  auto reduce = [&]() {
    reduce_max_async(colsum.p, (int64_t)n, res.p);    // (slab_norm's maximum: exact in any grouping)
    reduce_sum_pairs_async(part.p, n, res.p + 2);     // (slab_dot's two-level sum)
  };
  if (fold) {
    // (the operands' slots and per column the pads of a hull: what the kernel's per-column rule admits)
    const int64_t bound = fd.slots + fn.slots + 4LL * al * n;
    FreshSlabs fs(n, 1, bound, false, false);
    fs.why[0] = PT_WHY[0];
    fs.why[1] = PT_WHY[1];
    hull_slots(SlabIn<2>{{rd, rn}}, n, al, fs);
    hipLaunchKernelGGL(k_purify_tail<true>, grid, dim3(256), 0, stream(), n, rd, rn, rs, al, fs.base.p, fs.out(0), bound, colsum.p, part.p,
                       fs.stat.p);
    reduce();
    fs.also_fetch(res.p, 4, hr);
    DevMat R;
    if (!fs.finish("purify tail", D.rows, al, &R)) return false;
    bump_matrix_value_epoch();   // (the merge it replaces is in place: slab_axpby counts it so)
    Out = std::move(R);
  } else {
    DevBuf<unsigned long long> stat(1);
    stat.zero();
    hipLaunchKernelGGL(k_purify_tail<false>, grid, dim3(256), 0, stream(), n, rd, rn, rs, al, (const int64_t*)nullptr,
                       IsrOut{nullptr, nullptr, nullptr, nullptr, nullptr}, (int64_t)0, colsum.p, part.p, stat.p);
    reduce();
    unsigned long long hs = 0;
    {
      ScalarFetch ft;
      ft.add(stat.p, 1, &hs);
      ft.add(res.p, 4, hr);
      ft.run();
    }
    if (hs != 0) {
      pt_report(hs);
      return false;
    }
  }
  *norm = hr[1];
  dot[0] = hr[2];
  dot[1] = hr[3];
  return true;
}

}  // namespace ntp
