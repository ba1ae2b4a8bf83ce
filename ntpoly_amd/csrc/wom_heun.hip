// The tail of a Heun trial of the wave-operator-minimisation solvers (FermiOperatorModule.F90:358-398) on slab-form matrices,
// and the two dots of the canonical step (:484-507).  Between its products a trial builds, with the vocabulary at the solver's
// threshold,
//   RK2 = W;  RK2 += (h/2) K0;  RK2 += (h/2) K1;  Temp = RK1;  Temp += (-1) RK2;  err  = MatrixNorm(Temp)
//   Temp = RK2;  Temp += (-1) W;                                                  err2 = MatrixNorm(Temp)
// -- about thirteen reads and seven writes of runs the size of the iterate.  k_wom_heun reads the four runs once (columns of up
// to WOM_KC * 64 rows: once into registers; longer ones once per sweep) and writes RK2.
//
// Every merge is AddSparseVectors with its threshold as k_sa_axpby (kernels.hip) restates it on runs: the scaled addend is
// rounded, then added; a row both operands hold is kept when |sum| > thr; a row one operand holds is kept when |value| > thr,
// or unfiltered when it lies beyond the OTHER operand's last row.  In a chain of merges that "last row" is the last KEPT row
// of the link before, which is known only after the whole column of that link is decided -- hence three sweeps per column:
//   sweep 1:  M1  = W  + c K0             -> exh(M1)                          (c = h * 0.5 as the host rounds it)
//   sweep 2:  RK2 = M1 + c K1  (written)  -> exh(RK2), first, count
//   sweep 3:  D1  = RK1 - RK2,  D2 = RK2 - W  -> column sums of |D1|, |D2|
// The sweeps recompute the links before their own from the same inputs: the same expressions, the same bits.
//
// The norms steer the next step size, so they carry the bits of slab_norm on slab-form D1 / D2: k_sa_colstat gives lane t the
// rows first_kept + t + 64 m in ascending order, then runs the wave butterfly.  A lane of sweep 3 holds the rows of its own
// residue from the hull's first row b0 -- the same rows in the same order, dropped rows adding 0.0 -- so the 64 partial sums
// rotated by (first_kept - b0) & 63 go through the same butterfly.
//
// stat |= 1: a kept value of any link is exactly zero (compressed columns would store it, no run can); |= 2: runs far apart
// (the hull of W, K0, K1 is not bounded by their slots) or a slot beyond the output buffer -- nothing is written for that column.
#include <hip/hip_runtime.h>

#include "slab_columns.hpp"

namespace ntp {

int slab_wom_heun_register_rows() { return 512; }

namespace {
constexpr int WOM_KC = 8;   // chunks of 64 rows a column may span to be held in registers: 4 operands x 8 doubles per lane
static_assert(WOM_KC * WAVE == 512, "slab_wom_heun_register_rows() names the register path's bound");

// one row of B <- alpha A + B at thr (k_sa_axpby with beta = 1: B's value is read as it is); amax / bmax: the operands' last rows
// (-1: empty).  Returns the kept value, 0.0 for a row that is dropped or absent; *zk |= 1 when a kept value is exactly zero
__device__ inline double wom_link(double alpha, double a, double b, int r, int amax, int bmax, double thr, int* zk) {
  const bool ha = a != 0.0, hb = b != 0.0;
  const double wa = __dmul_rn(alpha, a);
  double o = 0.0;
  bool keep = false;
  if (ha && hb) { o = __dadd_rn(wa, b); keep = fabs(o) > thr; }
  else if (ha) { o = wa; keep = (r > bmax) ? true : (fabs(wa) > thr); }
  else if (hb) { o = b; keep = (r > amax) ? true : (fabs(b) > thr); }
  *zk |= (keep && o == 0.0) ? 1 : 0;
  return keep ? o : 0.0;
}

// the three sweeps of one column.  CACHED: the hull [b0, b1) of the four runs has at most WOM_KC * 64 rows and sits in registers,
// every load requested before the first sweep; otherwise each sweep reads the runs it needs again.
template <bool CACHED>
__device__ inline void wom_column(int j, int lane, const SlabCol<double>& cw, const SlabCol<double>& ck0, const SlabCol<double>& ck1,
                                  const SlabCol<double>& cr1, int a0, int a1, int b0, int b1, double c, double thr, double* __restrict__ dst,
                                  const IsrOut& o1, int64_t slot, double* __restrict__ cs1, double* __restrict__ cs2,
                                  unsigned long long* __restrict__ stat) {
  double w[WOM_KC], k0[WOM_KC], k1[WOM_KC], r1[WOM_KC];
  if (CACHED) {
#pragma unroll
    for (int k = 0; k < WOM_KC; ++k) {
      const int r = b0 + k * WAVE + lane;
      w[k] = slab_at(cw, r); k0[k] = slab_at(ck0, r); k1[k] = slab_at(ck1, r); r1[k] = slab_at(cr1, r);
    }
  }
  int zk = 0;
  // sweep 1: the last kept row of M1 = W + c K0 (IncrementMatrix(K0, RK2 = W, c, thr): A = K0, B = W)
  int e1 = -1;
  auto s1 = [&](int r, double vw, double vk0) {
    const double m1 = wom_link(c, vk0, vw, r, ck0.l, cw.l, thr, &zk);
    e1 = max(e1, m1 != 0.0 ? r : -1);
  };
  if (CACHED) {
#pragma unroll
    for (int k = 0; k < WOM_KC; ++k) s1(b0 + k * WAVE + lane, w[k], k0[k]);
  } else {
    for (int r = b0 + lane; r < b1; r += WAVE) s1(r, slab_at(cw, r), slab_at(ck0, r));
  }
  if (__ballot(zk != 0)) {   // (a kept zero of M1: its extent is not what compressed columns would carry on -- refused)
    if (lane == 0) {
      atomicOr(stat, 1ull);
      slab_empty_column(o1, j, slot);
      cs1[j] = 0.0; cs2[j] = 0.0;
    }
    return;
  }
  e1 = wave_max_i32(e1);
  // sweep 2: RK2 = M1 + c K1 (IncrementMatrix(K1, RK2, c, thr): A = K1, B = M1), written with its extent and count
  KeptExtent kept;
  auto s2 = [&](int r, double vw, double vk0, double vk1) {
    const double m1 = wom_link(c, vk0, vw, r, ck0.l, cw.l, thr, &zk);
    const double o = wom_link(c, vk1, m1, r, ck1.l, e1, thr, &zk);
    if (r >= a0 && r < a1) dst[r] = o;
    kept.note(o != 0.0, r);
  };
  if (CACHED) {
#pragma unroll
    for (int k = 0; k < WOM_KC; ++k) s2(b0 + k * WAVE + lane, w[k], k0[k], k1[k]);
  } else {
    for (int r = b0 + lane; r < b1; r += WAVE) s2(r, slab_at(cw, r), slab_at(ck0, r), slab_at(ck1, r));
  }
  kept.reduce();
  const int kl = kept.kl;
  // sweep 3: D1 = RK1 - RK2 (A = RK2, B = RK1) and D2 = RK2 - W (A = W, B = RK2): sums of moduli per lane residue, first kept rows
  double p1 = 0.0, p2 = 0.0;
  int f1 = INT_MAX, f2 = INT_MAX;
  auto s3 = [&](int r, double vw, double vk0, double vk1, double vr1) {
    const double m1 = wom_link(c, vk0, vw, r, ck0.l, cw.l, thr, &zk);
    const double o = wom_link(c, vk1, m1, r, ck1.l, e1, thr, &zk);
    const double d1 = wom_link(-1.0, o, vr1, r, kl, cr1.l, thr, &zk);
    const double d2 = wom_link(-1.0, vw, o, r, cw.l, kl, thr, &zk);
    p1 = __dadd_rn(p1, fabs(d1));
    p2 = __dadd_rn(p2, fabs(d2));
    f1 = min(f1, d1 != 0.0 ? r : INT_MAX);
    f2 = min(f2, d2 != 0.0 ? r : INT_MAX);
  };
  if (CACHED) {
#pragma unroll
    for (int k = 0; k < WOM_KC; ++k) s3(b0 + k * WAVE + lane, w[k], k0[k], k1[k], r1[k]);
  } else {
    for (int r = b0 + lane; r < b1; r += WAVE) s3(r, slab_at(cw, r), slab_at(ck0, r), slab_at(ck1, r), slab_at(cr1, r));
  }
  f1 = wave_min_i32(f1);
  f2 = wave_min_i32(f2);
  // (lane t of k_sa_colstat holds the rows first_kept + t + 64 m: the partial sum of lane (first_kept - b0 + t) & 63 here)
  const int rot1 = f1 == INT_MAX ? 0 : ((f1 - b0) & (WAVE - 1)), rot2 = f2 == INT_MAX ? 0 : ((f2 - b0) & (WAVE - 1));
  p1 = wave_sum_f64(__shfl(p1, (lane + rot1) & (WAVE - 1), WAVE));
  p2 = wave_sum_f64(__shfl(p2, (lane + rot2) & (WAVE - 1), WAVE));
  if (__ballot(zk != 0) && lane == 0) atomicOr(stat, 1ull);
  if (lane == 0) {
    kept.store(o1, j, slot, a0);
    cs1[j] = p1;
    cs2[j] = p2;
  }
}

// One wave per column.  base[j]: the slot of RK2's column (the aligned hull [a0, a1) of W, K0, K1, every row of it written: pads
// and dropped rows zero); cs1 / cs2: the column sums of |D1| / |D2|
__global__ __launch_bounds__(256) void k_wom_heun(int n, SlabRuns W, SlabRuns K0, SlabRuns K1, SlabRuns R1, double c, double thr, int al,
                                                  const int64_t* __restrict__ base, IsrOut o1, int64_t bound, double* __restrict__ cs1,
                                                  double* __restrict__ cs2, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const SlabCol<double> wk[3] = {slab_col<double>(W, j), slab_col<double>(K0, j), slab_col<double>(K1, j)}, cr1 = slab_col<double>(R1, j);
  const SlabCol<double> &cw = wk[0], &ck0 = wk[1], &ck1 = wk[2];
  const int64_t slot = base[j];
  const SlabHull h(wk, al);   // (of the three merged runs: RK1 joins the sweeps' hull below)
  const int a0 = h.a0, a1 = h.a1;
  // (runs far apart: their hull is not bounded by the three slots and the pads between them -- refused per column)
  if (h.apart(3, al) || slot + (int64_t)(a1 - a0) > bound) {
    if (lane == 0) {
      slab_empty_column(o1, j, slot);
      cs1[j] = 0.0; cs2[j] = 0.0;
      atomicOr(stat, 2ull);
    }
    return;
  }
  // the sweeps' hull takes RK1 in too (D1's rows); rows of it outside [a0, a1) hold no entry of RK2
  const int b0 = cr1.l >= 0 ? min(a0, cr1.f / al * al) : a0, b1 = cr1.l >= 0 ? max(a1, (cr1.l / al + 1) * al) : a1;
  double* __restrict__ dst = static_cast<double*>(o1.val) + (slot - a0);
  if (b1 - b0 <= WOM_KC * WAVE)
    wom_column<true>(j, lane, cw, ck0, ck1, cr1, a0, a1, b0, b1, c, thr, dst, o1, slot, cs1, cs2, stat);
  else
    wom_column<false>(j, lane, cw, ck0, ck1, cr1, a0, a1, b0, b1, c, thr, dst, o1, slot, cs1, cs2, stat);
}

// both dots of the canonical step, one wave per column: k_sa_dot's loop (from the later first row to the earlier last row of a
// pair, lane-strided, then the wave butterfly) on (X, W) into part1 and on (W, XA) into part2, as the (x, 0) pairs of its sum
__device__ inline double wom_pair_dot(const SlabCol<double>& a, const SlabCol<double>& b, int lane) {
  const int f = max(a.f, b.f), l = min(a.l, b.l);
  double s = 0.0;
  if (l >= f)
    for (int r = f + lane; r <= l; r += WAVE) s = __dadd_rn(s, __dmul_rn(a.p[r], b.p[r]));
  return wave_sum_f64(s);
}
__global__ __launch_bounds__(256) void k_wom_c_dots(int n, SlabRuns X, SlabRuns W, SlabRuns XA, double* __restrict__ part1,
                                                    double* __restrict__ part2) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const int lane = lane_id();
  const SlabCol<double> cx = slab_col<double>(X, j), cw = slab_col<double>(W, j), ca = slab_col<double>(XA, j);
  const double d1 = wom_pair_dot(cx, cw, lane), d2 = wom_pair_dot(cw, ca, lane);
  if (lane == 0) {
    part1[2 * (size_t)j] = d1; part1[2 * (size_t)j + 1] = 0.0;
    part2[2 * (size_t)j] = d2; part2[2 * (size_t)j + 1] = 0.0;
  }
}

}  // namespace

bool slab_wom_heun(const DevMat& W, const DevMat& K0, const DevMat& K1, const DevMat& RK1, double h, double thr, DevMat& Out, double* err,
                   double* err2) {
  const double c = h * 0.5;
  for (const DevMat* M : {&W, &K0, &K1, &RK1})
    if (!slab_merge_operand(*M, false)) return false;
  if (W.cols != K0.cols || W.cols != K1.cols || W.cols != RK1.cols || W.rows != K0.rows || W.rows != K1.rows || W.rows != RK1.rows || W.cols == 0)
    return false;
  if (!std::isfinite(h) || !std::isfinite(thr) || c == 0.0) return false;
  const SlabForm &fw = *W.slab, &f0 = *K0.slab, &f1 = *K1.slab, &fr = *RK1.slab;
  // (alignments that differ: the largest, where it is a multiple of the others, as the merge on runs takes them)
  const int n = W.cols, al = std::max(1, std::max(std::max(fw.row_pad, f0.row_pad), std::max(f1.row_pad, fr.row_pad)));
  for (const SlabForm* f : {&fw, &f0, &f1, &fr})
    if (al % std::max(1, f->row_pad) != 0) return false;
  // (the operands' slots and per column the pads of a hull: what k_wom_heun's per-column rule admits)
  const int64_t bound = fw.slots + f0.slots + f1.slots + 10LL * al * n;
  FreshSlabs fs(n, 1, bound, false, false);
  fs.why[0] = " a kept value is exactly zero";
  fs.why[1] = " runs far apart";
  DevBuf<double> cs1((size_t)n), cs2((size_t)n), res(4);
  const SlabRuns rw = slab_runs(W), r0 = slab_runs(K0), r1 = slab_runs(K1), rr = slab_runs(RK1);
  hull_slots(SlabIn<3>{{rw, r0, r1}}, n, al, fs);
  hipLaunchKernelGGL(k_wom_heun, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, rw, r0, r1, rr, c, thr, al, fs.base.p, fs.out(0), bound,
                     cs1.p, cs2.p, fs.stat.p);
  reduce_max_async(cs1.p, (int64_t)n, res.p);       // (slab_norm's maximum: exact in any grouping)
  reduce_max_async(cs2.p, (int64_t)n, res.p + 2);
  double hr[4] = {0.0, 0.0, 0.0, 0.0};
  fs.also_fetch(res.p, 4, hr);
  DevMat R;
  if (!fs.finish("wom heun", W.rows, al, &R)) return false;
  Out = std::move(R);
  *err = hr[1];
  *err2 = hr[3];
  return true;
}

bool slab_wom_c_dots(const DevMat& X, const DevMat& W, const DevMat& XA, double out[2]) {
  // (what slab_dot takes: zeros inside a run add exact zeros to the sums)
  auto ok = [](const DevMat& M) { return M.expanded() && !M.cplx && !M.slab->labelled() && (M.rows == M.cols || slab_panels_ok()); };
  if (!ok(X) || !ok(W) || !ok(XA) || X.cols != W.cols || X.cols != XA.cols || X.cols == 0) return false;
  const int n = X.cols;
  DevBuf<double> part1((size_t)2 * n), part2((size_t)2 * n), res(4);
  hipLaunchKernelGGL(k_wom_c_dots, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, slab_runs(X), slab_runs(W), slab_runs(XA), part1.p,
                     part2.p);
  reduce_sum_pairs_async(part1.p, n, res.p);       // (slab_dot's two-level sum)
  reduce_sum_pairs_async(part2.p, n, res.p + 2);
  double h[4] = {0.0, 0.0, 0.0, 0.0};
  ScalarFetch ft;
  ft.add(res.p, 4, h);
  ft.run();
  out[0] = h[0];
  out[1] = h[2];
  return true;
}

}  // namespace ntp
