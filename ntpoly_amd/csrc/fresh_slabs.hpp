// The output scaffold of the fused slab passes (slab_extra.hip: TRS4, the square-root chain, HPCP, ScaleAndFold, the transpose;
// and, with the input side of slab_columns.hpp, the chain passes, purify_tail.hip and wom_heun.hip): a pass that writes one or two fresh slab-form matrices launches its span kernel, scans the spans into slots,
// launches its chain kernel and ends in ONE host wait that brings back the kept counts, the slots used, the kernel's flags and the
// pass's sums.  Everything sits in an anonymous namespace: each translation unit gets its own copy, as with device_util.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "device_util.hpp"
#include "kernels.hpp"

namespace ntp {
namespace {
__global__ __launch_bounds__(256) void k_sa_count_sum(const int32_t* __restrict__ v, int n, unsigned long long* __restrict__ out) {
  __shared__ long long red[4];
  long long s = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s += v[i];
  s = wave_sum_i64(s);
  if (lane_id() == 0) red[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long t = red[0] + red[1] + red[2] + red[3];
    if (t) atomicAdd(out, (unsigned long long)t);
  }
}
// deterministic sum of n (a, b) pairs: fixed assignment of elements to threads, fixed tree -- the same bits every run
__global__ __launch_bounds__(256) void k_sa_sum_pairs(const double* __restrict__ in, int n, int chunk, double* __restrict__ out) {
  __shared__ double ra[256], rb[256];
  const int lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
  double a = 0.0, b = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    a = __dadd_rn(a, in[2 * (size_t)i]);
    b = __dadd_rn(b, in[2 * (size_t)i + 1]);
  }
  ra[threadIdx.x] = a;
  rb[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      ra[threadIdx.x] = __dadd_rn(ra[threadIdx.x], ra[threadIdx.x + o]);
      rb[threadIdx.x] = __dadd_rn(rb[threadIdx.x], rb[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = ra[0]; out[2 * blockIdx.x + 1] = rb[0]; }
}
void sum_pairs_async(const double* part, int n, double* out2) {
  const int chunk = 2048, g = cdiv(n, chunk);
  if (g <= 1) {
    hipLaunchKernelGGL(k_sa_sum_pairs, dim3(1), dim3(256), 0, stream(), part, n, std::max(n, 1), out2);
    return;
  }
  DevBuf<double> lvl((size_t)2 * g);
  hipLaunchKernelGGL(k_sa_sum_pairs, dim3(g), dim3(256), 0, stream(), part, n, chunk, lvl.p);
  hipLaunchKernelGGL(k_sa_sum_pairs, dim3(1), dim3(256), 0, stream(), lvl.p, g, g, out2);
}
struct IsrOut {   // one output: values into the slot at base[j], the kept extent and count per column
  void* val;
  int32_t* first;
  int32_t* last;
  int32_t* count;
  int64_t* off;
};
// The scaffold of a pass that writes one or two fresh slab-form matrices of n columns, `bound` entries (+ kIndexSlack) each.
// The pass launches its span kernel into `span`, calls scan(), launches its chain kernel on out(q), base, stat (and part, with
// sums), then finish(): the kept counts summed per output, the pairs of `part` summed, and the pass's one host wait.
// also_fetch(): words a pass reduced itself (a maximum, a sum in another kernel's order) ride on that same wait.
struct FreshSlabs {
  const int n, outs;
  const bool cplx;
  std::unique_ptr<SlabForm> fo[2];
  DevBuf<int32_t> span;
  DevBuf<int64_t> base;
  DevBuf<unsigned long long> stat, tot;
  DevBuf<double> part, res;   // (with sums only)
  const double* extra_dev = nullptr;
  double* extra_host = nullptr;
  int extra_words = 0;
  const char* why[2] = {" a scaled entry underflows to zero", " runs far apart"};   // what stat bits 1 and 2 mean to the pass (the debug line)
  FreshSlabs(int n_, int outs_, int64_t bound, bool cplx_, bool sums)
      : n(n_), outs(outs_), cplx(cplx_), span((size_t)n_), base((size_t)n_ + 1), stat(1), tot((size_t)outs_) {
    for (int q = 0; q < outs; ++q) {
      fo[q].reset(new SlabForm());
      fo[q]->first.alloc((size_t)n); fo[q]->last.alloc((size_t)n); fo[q]->count.alloc((size_t)n); fo[q]->off.alloc((size_t)n + 1);
      fo[q]->val.alloc(((size_t)bound + kIndexSlack) * (cplx ? 2 : 1));
    }
    if (sums) { part.alloc((size_t)2 * n); res.alloc(2); }
    stat.zero();
    tot.zero();
  }
  IsrOut out(int q) const {
    if (q >= outs) return IsrOut{nullptr, nullptr, nullptr, nullptr, nullptr};
    return IsrOut{fo[q]->val.p, fo[q]->first.p, fo[q]->last.p, fo[q]->count.p, fo[q]->off.p};
  }
  void scan() { scan_i32_async(span.p, base.p, (int64_t)n); }
  void also_fetch(const double* dev, int words, double* host) { extra_dev = dev; extra_words = words; extra_host = host; }
  // R[q]: the finished outputs of `rows` rows in slots aligned to `al`; sums: the first nsums sums of part's pairs.
  // false: the chain kernel set stat (1: a scaled entry underflows to zero, 2: a union extent beyond `bound`) -- nothing returned
  bool finish(const char* tag, int32_t rows, int al, DevMat* R, double* sums = nullptr, int nsums = 0) {
    const dim3 sum_grid(std::max(1, std::min(256, cdiv(n, 1024))));
    for (int q = 0; q < outs; ++q) hipLaunchKernelGGL(k_sa_count_sum, sum_grid, dim3(256), 0, stream(), fo[q]->count.p, n, tot.p + q);
    if (nsums) sum_pairs_async(part.p, n, res.p);
    int64_t nnz[2] = {0, 0}, slots = 0;
    unsigned long long hs = 0;
    {
      ScalarFetch ft;
      ft.add(tot.p, outs, nnz);
      ft.add(base.p + n, 1, &slots);
      ft.add(stat.p, 1, &hs);
      if (nsums) ft.add(res.p, nsums, sums);
      if (extra_words) ft.add(extra_dev, extra_words, extra_host);
      ft.run();
    }
    if (hs != 0) {   // (the caller takes the vocabulary calls)
      if (std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
        std::fprintf(stderr, "[%s] refused:%s%s\n", tag, (hs & 1ull) ? why[0] : "", (hs & 2ull) ? why[1] : "");
      return false;
    }
    for (int q = 0; q < outs; ++q) {
      fo[q]->row_pad = al;
      fo[q]->slots = slots;
      R[q].rows = rows; R[q].cols = n; R[q].cplx = cplx; R[q].nnz = nnz[q]; R[q].zero_free = 1;
      R[q].slab = std::move(fo[q]);
    }
    return true;
  }
};
}  // namespace
}  // namespace ntp
