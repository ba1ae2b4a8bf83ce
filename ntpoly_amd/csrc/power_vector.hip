// PowerBounds on one vector (option power_vector): the reference's power iteration carries an N x N matrix
// whose N columns are the same vector and stay the same, so the loop of solvers_func.cpp carries ONE column as a dense array
// and a step is a sparse matrix-vector product with the arithmetic of the engine's SpGEMM on that column.
//
// Gather form of A (PowerGather, built once per solve from the compressed columns of A: for every row i the pairs (k, A(i, k))
// in ascending k, what transpose() produces): slices of 64 rows, column-major within a slice -- entry t of rows 64 s .. 64 s + 63 lies at soff[s] + 64 t + (row & 63),
// 64-bit offsets per slice, a slice padded to its longest row.  A wave with one lane per row reads consecutive addresses
// while every lane walks its own row in order.  The padding is stored as (k = 0, a = 0) so that every address of a slice is
// readable, and it is MASKED by the row's length: a lane never feeds a padding slot into its chain.
//
// k_pv_step: y_i = the chain over ascending k of A(i, k) x(k) -- Sc<T>::fmadd, what every product kernel of the engine
// computes for an entry (real FMA mode: fma(a, x, acc); real unfused: a rounded product, then a rounded add; complex: the
// reference's complex multiply-add) -- then the product's pruning rule (|y_i| > threshold, strict, the modulus for complex;
// otherwise 0), and per workgroup the partial sums of conj(x) x, Re conj(x) y and |y| in a fixed order (wave butterfly, then
// the waves in order through LDS).  k_pv_finish sums the partials in a fixed order: no floating-point atomics, the same
// input gives the same three numbers on every run.  k_pv_scale: x <- y * (1 / n1), pruned slots stay 0.
// Several ranks: a rank's gather form holds the k of its own column panel, k_pv_step<., ., false> leaves the partial chains,
// the transport sums them, and k_pv_tail prunes and reduces the full vector identically on every rank.
#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "device_util.hpp"
#include "kernels.hpp"

namespace ntp {
namespace {

constexpr int PV_NW = 4;   // waves (= slices) per workgroup

// The rows of A from its compressed columns.  The entries of a column lie at ascending positions p and columns follow each
// other, so a STABLE sort of the positions by row index lists every row's entries in ascending k -- what transpose() produces,
// with 32-bit keys over the bits of n and 16 bytes per entry of sort buffers instead of its 64-bit keys.
// row lengths: integer atomics (a count does not depend on their order); the sort's keys and payload
__global__ void k_pv_count(const int32_t* __restrict__ inner, int64_t nnz, int32_t* __restrict__ len, unsigned int* __restrict__ keys,
                           unsigned int* __restrict__ pos) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
    const int r = inner[p];
    atomicAdd(&len[r], 1);
    keys[p] = (unsigned int)r;
    pos[p] = (unsigned int)p;
  }
}

// one wave per slice: the slice's width (its longest row)
__global__ __launch_bounds__(PV_NW* WAVE) void k_pv_widths(int nslices, const int32_t* __restrict__ len, int32_t* __restrict__ width) {
  const int s = blockIdx.x * PV_NW + threadIdx.x / WAVE;
  if (s >= nslices) return;
  const int w = wave_max_i32(len[s * WAVE + lane_id()]);   // (len has nslices * 64 entries, 0 beyond n)
  if (lane_id() == 0) width[s] = w;
}

// one lane per row: entry t of row r is position sorted[rowstart[r] + t] of A's columns; its column by bisection of outer
template <typename T>
__global__ __launch_bounds__(PV_NW* WAVE) void k_pv_fill(Csc A, int n, int nslices, int koff, const int32_t* __restrict__ len,
                                                         const int64_t* __restrict__ rowstart, const unsigned int* __restrict__ sorted,
                                                         const int64_t* __restrict__ soff, int32_t* __restrict__ idx, T* __restrict__ val) {
  const int s = blockIdx.x * PV_NW + threadIdx.x / WAVE;
  if (s >= nslices) return;
  const int lane = lane_id();
  const int row = s * WAVE + lane;
  const int l = len[row];
  const int64_t base = soff[s];
  const int w = (int)((soff[s + 1] - base) / WAVE);
  const int64_t r0 = row < n ? rowstart[row] : 0;
  const T* __restrict__ Av = static_cast<const T*>(A.val);
  int lo = 0;   // (a row's columns ascend: the search starts at the last one found)
  for (int t = 0; t < w; ++t) {
    const int64_t q = base + (int64_t)t * WAVE + lane;
    int k = 0;
    T v = Sc<T>::zero();
    if (t < l) {
      const int64_t p = (int64_t)sorted[r0 + t];
      int hi = A.cols;   // the column j in [lo, hi) with outer[j] <= p < outer[j + 1]
      while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (A.outer[mid] <= p) lo = mid;
        else hi = mid;
      }
      k = lo + koff;
      v = Av[p];
    }
    idx[q] = k;
    val[q] = v;
  }
}

__device__ inline double pv_conj_dot(double a, double b) { return __dmul_rn(a, b); }   // Re conj(a) b
__device__ inline double pv_conj_dot(double2 a, double2 b) { return __dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)); }

// prune acc, store it, and leave the workgroup's three partial sums in part[3 b ..]: lanes of a wave by the xor butterfly,
// the waves in order -- the same order on every run
template <typename T>
__device__ inline void pv_tail(T acc, bool valid, int row, const T* __restrict__ x, T* __restrict__ y, double threshold,
                               double* __restrict__ part) {
  __shared__ double red[PV_NW][3];
  const bool keep = valid && Sc<T>::mag(acc) > threshold;
  const T yv = keep ? acc : Sc<T>::zero();
  const T xv = valid ? x[row] : Sc<T>::zero();
  if (valid) y[row] = yv;
  const double d1 = wave_sum_f64(pv_conj_dot(xv, xv));
  const double d2 = wave_sum_f64(pv_conj_dot(xv, yv));
  const double n1 = wave_sum_f64(keep ? Sc<T>::mag(yv) : 0.0);
  const int wave = threadIdx.x / WAVE;
  if (lane_id() == 0) {
    red[wave][0] = d1;
    red[wave][1] = d2;
    red[wave][2] = n1;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < PV_NW; ++w) s = __dadd_rn(s, red[w][threadIdx.x]);
    part[(size_t)blockIdx.x * 3 + threadIdx.x] = s;
  }
}

// one lane per row.  TAIL: prune and reduce here (one rank); otherwise y = the partial chains of this rank's panel
template <typename T, bool FMA, bool TAIL>
__global__ __launch_bounds__(PV_NW* WAVE) void k_pv_step(int n, int nslices, const int32_t* __restrict__ len, const int64_t* __restrict__ soff,
                                                         const int32_t* __restrict__ idx, const T* __restrict__ val, const T* __restrict__ x,
                                                         T* __restrict__ y, double threshold, double* __restrict__ part) {
  const int s = blockIdx.x * PV_NW + threadIdx.x / WAVE;   // (wave-uniform; a wave past the last slice only joins the reduction)
  const int lane = lane_id();
  const int row = s * WAVE + lane;
  const bool valid = s < nslices && row < n;
  T acc = Sc<T>::zero();
  if (s < nslices) {
    const int l = len[row];
    const int64_t base = soff[s] + lane;
    const int w = (int)((soff[s + 1] - soff[s]) / WAVE);
    constexpr int U = 4;   // entries of a row in flight together: index, then value and x(k)
    for (int t0 = 0; t0 < w; t0 += U) {
      int k[U];
      T a[U], b[U];
      bool in[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        in[u] = t0 + u < l;
        k[u] = in[u] ? idx[base + (int64_t)(t0 + u) * WAVE] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = in[u] ? val[base + (int64_t)(t0 + u) * WAVE] : Sc<T>::zero();
        b[u] = in[u] ? x[k[u]] : Sc<T>::zero();
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (in[u]) acc = Sc<T>::fmadd(a[u], b[u], acc, FMA);
    }
  }
  if (TAIL) pv_tail<T>(acc, valid, row, x, y, threshold, part);
  else if (valid) y[row] = acc;
}

// several ranks: y holds the sums of the ranks' partial chains; prune in place and reduce
template <typename T>
__global__ __launch_bounds__(PV_NW* WAVE) void k_pv_tail(int n, const T* __restrict__ x, T* __restrict__ y, double threshold, double* __restrict__ part) {
  const int row = blockIdx.x * (PV_NW * WAVE) + threadIdx.x;
  const bool valid = row < n;
  pv_tail<T>(valid ? y[row] : Sc<T>::zero(), valid, row, x, y, threshold, part);
}

// out = (d1, d2, n1, 1 / n1): thread t sums the partials t, t + 256, ... in order, then a fixed tree through LDS
__global__ __launch_bounds__(256) void k_pv_finish(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double red[3][256];
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblocks; b += 256)
    for (int q = 0; q < 3; ++q) s[q] = __dadd_rn(s[q], part[(size_t)b * 3 + q]);
  for (int q = 0; q < 3; ++q) red[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] = __dadd_rn(red[q][threadIdx.x], red[q][threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = red[0][0];
    out[1] = red[1][0];
    out[2] = red[2][0];
    out[3] = 1.0 / red[2][0];
  }
}

// x <- y * s, the one multiplication of ScaleMatrix on every part of an entry; a pruned slot stays 0 (also when s is not finite)
template <typename T>
__global__ void k_pv_scale(int n, const T* __restrict__ y, const double* __restrict__ out, T* __restrict__ x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T v = y[i];
  x[i] = Sc<T>::is_zero(v) ? Sc<T>::zero() : Sc<T>::scale(out[3], v);
}

}  // namespace

bool power_gather_build(const DevMat& A, int32_t koff, PowerGather& G) {
  // (A: the compressed columns of this rank's panel -- all n rows, the panel's columns; koff = its first column)
  const int64_t n64 = A.rows, nnz = A.nnz;
  if (n64 <= 0 || (int64_t)koff + A.cols > (int64_t)INT32_MAX || n64 + WAVE > (int64_t)INT32_MAX || nnz > (int64_t)INT32_MAX) return false;
  const int n = A.rows;
  const int nslices = cdiv(n, WAVE);
  // the allocations must succeed: the allocator is fatal when the device is full, so ask first -- 16 bytes per entry for the
  // sort, then 12 (complex: 20) per padded entry, of which there are at least nnz; the padding is checked below
  const size_t per = 4 + 8 * A.wval();
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (2 * (size_t)nnz * (16 + per) > free_b + dev_bytes_cached()) return false;
  G.n = n;
  G.cplx = A.cplx;
  G.nslices = nslices;
  G.len.alloc((size_t)nslices * WAVE);
  G.len.zero();
  DevBuf<int32_t> width((size_t)nslices);
  DevBuf<int64_t> rowstart((size_t)n + 1);
  DevBuf<unsigned int> sorted;   // the positions of A's entries, by row and within a row ascending
  const Csc a = view(A);
  if (nnz > 0) {
    DevBuf<unsigned int> keys((size_t)nnz), keys2((size_t)nnz), pos((size_t)nnz), pos2((size_t)nnz);
    hipLaunchKernelGGL(k_pv_count, dim3(std::min(cdiv(nnz, 256), 8192)), dim3(256), 0, stream(), A.inner.p, nnz, G.len.p, keys.p, pos.p);
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n64) ++bits;
    rocprim::double_buffer<unsigned int> kb(keys.p, keys2.p), pb(pos.p, pos2.p);
    size_t tmp_bytes = 0;
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, pb, (size_t)nnz, 0, bits, stream()));
    DevBuf<char> tmp(tmp_bytes);
    HIP_CHECK(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, kb, pb, (size_t)nnz, 0, bits, stream()));
    sorted = pb.current() == pos.p ? std::move(pos) : std::move(pos2);
    // (keys, keys2 and the other payload buffer go back to the pool here: the form's arrays take their blocks)
  }
  hipLaunchKernelGGL(k_pv_widths, dim3(cdiv(nslices, PV_NW)), dim3(PV_NW * WAVE), 0, stream(), nslices, G.len.p, width.p);
  scan_i32_async(G.len.p, rowstart.p, (int64_t)n);
  std::vector<int32_t> hw((size_t)nslices);
  width.download(hw.data(), (size_t)nslices);
  std::vector<int64_t> hoff((size_t)nslices + 1);
  hoff[0] = 0;
  for (int s = 0; s < nslices; ++s) hoff[(size_t)s + 1] = hoff[(size_t)s] + (int64_t)hw[(size_t)s] * WAVE;
  const int64_t entries = hoff[(size_t)nslices];
  // (a slice is padded to its longest row: one full row among empty ones costs 64 times its length)
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (2 * (size_t)entries * per > free_b + dev_bytes_cached()) return false;
  G.entries = entries;
  G.soff.alloc((size_t)nslices + 1);
  G.soff.upload(hoff.data(), (size_t)nslices + 1);
  G.idx.alloc((size_t)entries);
  G.val.alloc((size_t)entries * A.wval());
  dispatch_type(A.cplx, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_pv_fill<T>), dim3(cdiv(nslices, PV_NW)), dim3(PV_NW * WAVE), 0, stream(), a, n, nslices, (int)koff, G.len.p, rowstart.p,
                       sorted.p, G.soff.p, G.idx.p, reinterpret_cast<T*>(G.val.p));
  });
  sync_stream();   // (hoff is read by the upload until here)
  return true;
}

int power_vector_blocks(int32_t n) { return cdiv(cdiv(n, WAVE), PV_NW); }

void power_vector_chains(const PowerGather& G, const double* x, double* y, double threshold, bool fma, bool tail, double* part) {
  const int nb = power_vector_blocks(G.n);
  dispatch_type(G.cplx, [&](auto tag) {
    using T = decltype(tag);
    const T* xv = reinterpret_cast<const T*>(x);
    const T* av = reinterpret_cast<const T*>(G.val.p);
    T* yv = reinterpret_cast<T*>(y);
#define NTP_PV_LAUNCH(FMA, TAIL)                                                                                                              \
  hipLaunchKernelGGL((k_pv_step<T, FMA, TAIL>), dim3(nb), dim3(PV_NW * WAVE), 0, stream(), G.n, G.nslices, G.len.p, G.soff.p, G.idx.p, av, xv, yv, \
                     threshold, part)
    if (fma && tail) NTP_PV_LAUNCH(true, true);
    else if (fma) NTP_PV_LAUNCH(true, false);
    else if (tail) NTP_PV_LAUNCH(false, true);
    else NTP_PV_LAUNCH(false, false);
#undef NTP_PV_LAUNCH
  });
}

void power_vector_tail(int32_t n, bool cplx, const double* x, double* y, double threshold, double* part) {
  dispatch_type(cplx, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_pv_tail<T>), dim3(power_vector_blocks(n)), dim3(PV_NW * WAVE), 0, stream(), (int)n, reinterpret_cast<const T*>(x),
                       reinterpret_cast<T*>(y), threshold, part);
  });
}

void power_vector_finish(int32_t n, const double* part, double* out) {
  hipLaunchKernelGGL(k_pv_finish, dim3(1), dim3(256), 0, stream(), part, power_vector_blocks(n), out);
}

void power_vector_scale(int32_t n, bool cplx, const double* y, const double* out, double* x) {
  dispatch_type(cplx, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_pv_scale<T>), dim3(cdiv(n, 256)), dim3(256), 0, stream(), (int)n, reinterpret_cast<const T*>(y), out,
                       reinterpret_cast<T*>(x));
  });
}

}  // namespace ntp
