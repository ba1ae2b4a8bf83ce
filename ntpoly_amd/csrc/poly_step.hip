// The tail of a step of the Chebyshev / Hermite recurrences (ChebyshevSolversModule.F90:69-160, HermiteSolversModule.F90:52-184)
// on real slab-form matrices.  Behind the product P = 2 X T(k-1) a step makes, with the vocabulary at threshold 0,
//   IncrementMatrix(Q, P, a, 0)    Tk = P + a Q       (Q = T(k-2), a = -1)
//   IncrementMatrix(Tk, R, c, 0)   R' = R + c Tk      (R the running sum)
// -- six matrix-sized streams and two read-backs.  k_poly_step reads the runs of P, Q and R once and writes Tk and R': five streams
// and one read-back, and Tk goes from the first merge into the second in a register.
//
// The rules of a merge and of the stat bits, and the sweep itself (hull_sweep), are in slab_columns.hpp: a row that cancels in the
// first merge is ABSENT for the second, and a lane needs nothing but its own row of Tk.
#include <hip/hip_runtime.h>

#include "slab_columns.hpp"

namespace ntp {
namespace {
// x = (P, Q, R) of a row; output 0 = Tk, 1 = R'.  Stat bit 1: a zero scaled value wherever the addend is held, as SumRow (sum_chain.hip) --
// not PadeRow's rule (pade_chain.hip)
struct PolyRow {
  double a, c;
  template <typename Emit>
  __device__ inline void operator()(const double (&x)[3], const Emit& emit, int& zk) const {
    // IncrementMatrix(Q, P, a, 0): Q the addend, P the running value
    const bool hq = x[1] != 0.0;
    const double wq = Sc<double>::scale(a, x[1]);
    zk |= (hq && wq == 0.0) ? 1 : 0;
    double t = x[0];
    bool ht = x[0] != 0.0;
    merge0(wq, hq, t, ht);
    t = ht ? t : 0.0;
    // IncrementMatrix(Tk, R, c, 0): Tk the addend, from the register; R the running value
    const double wt = Sc<double>::scale(c, t);
    zk |= (ht && wt == 0.0) ? 1 : 0;
    double v = x[2];
    bool hv = x[2] != 0.0;
    merge0(wt, ht, v, hv);
    emit(0, t, ht);
    emit(1, hv ? v : 0.0, hv);
  }
};

__global__ __launch_bounds__(256) void k_poly_step(int n, SlabIn<3> P, PolyRow row, int al, const int64_t* __restrict__ base, IsrOut ot, IsrOut orr,
                                                   int64_t bound, unsigned long long* __restrict__ stat) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (j >= n) return;
  const IsrOut out[2] = {ot, orr};
  hull_sweep<double>(j, lane_id(), P, row, al, base, out, bound, stat);
}
}  // namespace

bool slab_poly_step(const DevMat& P, const DevMat& Q, const DevMat& R, double a, double c, DevMat& Tk, DevMat& Rout) {
  const DevMat* in[3] = {&P, &Q, &R};
  int al = 1;
  for (int k = 0; k < 3; ++k) {
    if (!slab_merge_operand(*in[k], false)) return false;
    al = std::max(al, in[k]->slab->row_pad);
  }
  if (!same_frame(in, 3, false) || P.cols == 0) return false;
  // (the outputs' slots are aligned to the widest alignment of the inputs, which has to hold every input's own)
  for (int k = 0; k < 3; ++k)
    if (al % std::max(1, in[k]->slab->row_pad) != 0) return false;
  if (!scalar_usable(a) || !scalar_usable(c)) return false;
  const int n = P.cols;
  SlabIn<3> I;
  // (the operands' slots, re-aligned to al, and per column the pads of a hull: what the kernel's per-column rule admits)
  const int64_t bound = slab_in(in, I) + 9LL * al * n;
  FreshSlabs fs(n, 2, bound, false, false);
  fs.why[0] = SLAB_WHY_ZERO;
  fs.why[1] = SLAB_WHY_APART;
  hull_slots(I, n, al, fs);
  hipLaunchKernelGGL(k_poly_step, dim3(cdiv((int64_t)n * WAVE, 256)), dim3(256), 0, stream(), n, I, PolyRow{a, c}, al, fs.base.p, fs.out(0), fs.out(1),
                     bound, fs.stat.p);
  DevMat O[2];
  if (!fs.finish("poly step", P.rows, al, O)) return false;
  Tk = std::move(O[0]);
  Rout = std::move(O[1]);
  return true;
}

}  // namespace ntp
