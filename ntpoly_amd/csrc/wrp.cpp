// C ABI of the engine: the reference's own wrapper surface (Source/Wrapper/*_wrp.F90, declared in
// Source/C/*_c.h) re-exported with identical names, argument order and calling convention
// (every scalar by reference, handles = caller-owned int[SIZE_wrp] buffers, no status codes),
// plus a few ntpoly_amd_* extension entry points (RCCL bootstrap, statistics, options).
// See include/*.h for the declarations with the reference line each symbol replaces.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.hpp"
#include "spgemm_block.hpp"
#include "spgemm_tile.hpp"
#include "io.hpp"

using namespace ntp;

namespace {
constexpr int SIZE_wrp = 12;  // Source/C/Wrapper.h:4

template <typename T>
T* get(const int* ih) {
  T* p;
  std::memcpy(&p, ih, sizeof(p));
  if (!p) NTP_FATAL("null handle passed to the C ABI");
  return p;
}
PSMatrix* get_unpacked(const int* ih) {
  PSMatrix* p;
  std::memcpy(&p, ih, sizeof(p));
  if (!p) NTP_FATAL("null handle passed to the C ABI");
  return p;
}
// every entry point sees packed matrices; only the TRS2 step below passes its iterate on as it is (kernels.hpp, pack())
template <>
PSMatrix* get<PSMatrix>(const int* ih) {
  PSMatrix* p = get_unpacked(ih);
  if (p->loc.loose() || p->loc.expanded() || p->loc.blocked()) pack(p->loc);
  return p;
}
// The vocabulary entry points (MatrixMultiply, IncrementMatrix, ScaleMatrix, CopyMatrix, DotMatrix, MatrixNorm) run
// inside a slab session of their own (engine.hpp SlabSession; FMA arithmetic, one rank, real -- complex ones in block form where
// complex sessions and the complex block path are allowed, psmatrix.cpp complex_blocks_on; option slab_algebra):
// a caller's own loop over the C ABI then keeps its matrices in the tile kernel's operand form between its calls --
// operands are converted where they are on first use, products stay where the kernel wrote them -- and every OTHER
// entry point still sees compressed columns (get<PSMatrix> packs on access).  Session not open: packed as ever.
// The session is judged on the communicator of the call's first matrix operand: its scope is declared first, so it is
// open before the session is.
struct ApiSession {
  CommScope cs;
  SlabSession s;
  explicit ApiSession(const int* ih_first) : cs(get_unpacked(ih_first)->grid), s(true, true) {}
  PSMatrix* mat(const int* ih) const { return s.opened ? get_unpacked(ih) : get<PSMatrix>(ih); }
};
template <typename T>
void put(int* ih, T* p) {
  std::memset(ih, 0, sizeof(int) * SIZE_wrp);
  std::memcpy(ih, &p, sizeof(p));
}

struct Pool {  // MatrixMemoryPool_p / _lr / _lc: the engine keeps its own HBM workspace
  int dummy = 0;
};
struct LocalMat {  // Matrix_lsr / Matrix_lsc
  DevMat m;
};

const ProcessGrid* default_grid() {
  if (!global_grid_constructed()) NTP_FATAL("the global process grid has not been constructed");
  return &global_grid();
}
std::string fstring(const char* s, const int* n) { return std::string(s, (size_t)*n); }

// MatrixDiagonalScale of a local matrix (sparse_includes/MatrixDiagonalScale.f90): values of column `index_column`
// are multiplied by the triplet's value, triplet after triplet
void local_diagonal_scale(DevMat& m, const HostTriplets& t) {
  if (m.cols == 0) return;
  const size_t w = m.wval();
  std::vector<double> f((size_t)m.cols * w, 0.0);
  for (int32_t j = 0; j < m.cols; ++j) f[(size_t)j * w] = 1.0;
  for (size_t i = 0; i < t.size(); ++i) {
    const int32_t col = t.col[i] - 1;
    if (col < 0 || col >= m.cols) continue;
    const double re = t.cplx ? t.val[2 * i] : t.val[i], im = t.cplx ? t.val[2 * i + 1] : 0.0;
    double& fr = f[(size_t)col * w];
    if (m.cplx) {
      double& fi = f[(size_t)col * w + 1];
      const double nr = fr * re - fi * im, ni = fr * im + fi * re;
      fr = nr;
      fi = ni;
    } else {
      fr *= re;
    }
  }
  DevBuf<double> d(f.size());
  d.upload(f.data(), f.size());
  scale_columns(m, d.p);
  sync_stream();
}
// PrintMatrix (sparse_includes/PrintMatrix.f90): MatrixMarket coordinate text, entries in column order
void local_print(const DevMat& m, const char* path) {
  HostTriplets t;
  to_triplets(m, 0, t);
  FILE* f = path ? std::fopen(path, "w") : stdout;
  if (!f) NTP_FATAL(std::string("cannot open ") + path + " for writing");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate %s general\n%%\n", m.cplx ? "complex" : "real");
  std::fprintf(f, "%d %d %lld\n", m.rows, m.cols, (long long)m.nnz);
  for (size_t i = 0; i < t.size(); ++i) {
    if (m.cplx) std::fprintf(f, "%d %d %.17g %.17g\n", t.row[i], t.col[i], t.val[2 * i], t.val[2 * i + 1]);
    else std::fprintf(f, "%d %d %.17g\n", t.row[i], t.col[i], t.val[i]);
  }
  if (path) std::fclose(f);
  else std::fflush(f);
}
std::unique_ptr<SlabSession> g_test_session;   // (ntpoly_amd_session_begin / _end: a diagnostic surface)
// the field of options() that the option table (kernels.hpp option_table) lists under this name
int& option_field(const char* name) {
  for (const OptionEntry& o : option_table)
    if (std::strcmp(o.name, name) == 0) return options().*o.field;
  NTP_FATAL("unknown option " + std::string(name));
}
}  // namespace

extern "C" {

// ===================================================================== extensions
// RCCL bootstrap: rank 0 calls ntpoly_amd_get_unique_id, the launcher broadcasts the 128 bytes,
// every rank calls ntpoly_amd_init_comm before constructing a process grid.
void ntpoly_amd_get_unique_id(char* out128) { comm_get_unique_id(out128); }
void ntpoly_amd_init_comm(const char* id128, const int* rank, const int* nranks) { comm_init(id128, *rank, *nranks); }
void ntpoly_amd_finalize_comm() { comm_finalize(); }
int ntpoly_amd_comm_rank() { return base_world().rank; }
int ntpoly_amd_comm_size() { return base_world().nranks; }
void ntpoly_amd_barrier() { comm_barrier(); }   // (all processes: no scope is open here)
// max over all ranks of n host doubles, in place (timing of a distributed region: the slowest rank counts)
void ntpoly_amd_allreduce_max(double* values, const int* n) { comm_allreduce_max(values, *n); }
void ntpoly_amd_synchronize() {
  ensure_init();
  sync_stream();
  HIP_CHECK(hipDeviceSynchronize());
}
// number of visible GPUs (0 without failing: used by test collection)
int ntpoly_amd_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
void ntpoly_amd_panel_range(const int* dim, const int* nranks, const int* rank, int* c0, int* c1) {
  panel_range(*dim, *nranks, *rank, c0, c1);
}
// columns [a, b) of rank s's panel that a requester whose B panel has rows [kmin, kmax] receives
void ntpoly_amd_halo_segment(const int* dim, const int* nranks, const int* s, const int* kmin, const int* kmax, int* a,
                             int* b) {
  halo_segment(*dim, *nranks, *s, *kmin, *kmax, a, b);
}
// the layout of one panel exchange on rank `me` (psmatrix.cpp panel_exchange_layout: the host arithmetic of the halo exchange of
// the fused panel steps): req = 4 words per rank (first, last row of its panel of B, two unused here), cnt[s P + q] = doubles
// rank s sends to rank q
void ntpoly_amd_panel_exchange_layout(const int* dim, const int* nranks, const int* me, const long long* req, const long long* cnt,
                                      int* sa, int* sb, long long* soff, int* ra, int* rb, long long* zoff) {
  panel_exchange_layout(*dim, *nranks, *me, reinterpret_cast<const int64_t*>(req), reinterpret_cast<const int64_t*>(cnt), sa, sb,
                        reinterpret_cast<int64_t*>(soff), ra, rb, reinterpret_cast<int64_t*>(zoff));
}
// every option of csrc/options.inc by its name; an unknown name is fatal
void ntpoly_amd_set_option(const char* name, const int* value) { option_field(name) = *value; }
// the current value of an option (bench.py prints the arithmetic a drop-in caller gets)
int ntpoly_amd_get_option(const char* name) { return option_field(name); }
// ntpoly_amd_<name>_counts(out) for every entry of csrc/counters.inc, where the slots are documented
#define NTP_COUNTER(name, N, accessor) \
  void ntpoly_amd_##name##_counts(long long out[N]) { std::copy_n(accessor(), N, out); }
#include "counters.inc"
#undef NTP_COUNTER
// (not in counters.inc: fields of a struct and two timings, not a counter array)
// statistics of the last SpGEMM: out[0..12]: nnzA, nnzB, nnzC, products, tmp_entries, bins[6], overflow, slab kernel used
void ntpoly_amd_last_spgemm_stats(long long* out, float* ms_numeric, float* ms_total) {
  flush_spgemm_timers();
  const SpgemmStats& s = last_spgemm_stats();
  out[0] = s.nnz_a; out[1] = s.nnz_b; out[2] = s.nnz_c; out[3] = s.products; out[4] = s.tmp_entries;
  for (int i = 0; i < 6; ++i) out[5 + i] = s.bin_cols[i];
  out[11] = s.overflow_cols;
  out[12] = s.slab;
  *ms_numeric = s.ms_numeric;
  *ms_total = s.ms_total;
}
// (not in counters.inc: fields of the same struct and a ratio)
// grouped LDS-hash path of the last SpGEMM: out[0..5] = used, columns handed back to the per-column kernels, groups,
// table class, min-hash clustering used, steps (sum of the groups' row unions of B); ratio = steps / (nnz(B) / columns per group)
void ntpoly_amd_last_grouped_stats(long long* out, double* ratio) {
  const SpgemmStats& s = last_spgemm_stats();
  out[0] = s.grouped; out[1] = s.gh_failed_cols; out[2] = s.gh_groups; out[3] = s.gh_level; out[4] = s.gh_minhash;
  out[5] = s.gh_tile_rows;
  *ratio = s.gh_union_ratio;
}
// forgets what the grouped path keeps between products (kept column orders, table class hints, "grouped kernel first"
// dimensions): the class a product starts in then does not depend on earlier products of the process
void ntpoly_amd_drop_grouped_caches() { drop_grouped_caches(); }
// 1: the last SpGEMM ran on the thin-left kernel (spgemm_thin.hip)
int ntpoly_amd_last_spgemm_thin() { return last_spgemm_stats().thin; }
// DIAGNOSTIC surface (like ntpoly_amd_trs2_step): a session of the kind the solver loops open (engine.hpp SlabSession), held
// open across the vocabulary calls that follow -- MatrixMultiply, IncrementMatrix, ScaleMatrix, CopyMatrix keep their
// matrices in slab form between the calls; *complex_ok != 0: complex operands too, which the one-call sessions of the C ABI
// do not take in slab form.  Every other entry point still sees compressed columns (it packs on access).  Tests reach the
// session kernels with operands of their own this way; one session at a time, ended by ntpoly_amd_session_end.
void ntpoly_amd_session_begin(const int* complex_ok) {
  if (g_test_session) NTP_FATAL("ntpoly_amd_session_begin: a session is already open");
  g_test_session.reset(new SlabSession(true, false, *complex_ok != 0));
}
void ntpoly_amd_session_end() { g_test_session.reset(); }
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin (complex_ok) and _end: the fused recurrence step of the
// Chebyshev / Hermite loops on caller-held complex matrices (engine.hpp ps_recurrence_step: Tk = P + a Tkm2, R <- R + c Tk);
// returns 1 when the step was taken, 0 when it declined and left every matrix as it was
int ntpoly_amd_recurrence_step(const int* ih_P, const int* ih_Tkm2, int* ih_Tk, int* ih_R, const double* a, const double* c) {
  return ps_recurrence_step(*get_unpacked(ih_P), *get_unpacked(ih_Tkm2), *get_unpacked(ih_Tk), *get_unpacked(ih_R), *a, *c) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end: one fused chain on caller-held matrices X and X2 (what
// the loop's product X X would be), real or -- in a session with complex_ok -- complex.  The two operands are brought into slab
// form, the chain of *order (5 or 3) runs, the outputs are packed into the result handles: order 5: Out1 = (X2 + a X) + (X + b I)
// and Out2 = (X2 + a X) + c I; order 3: Out1 = 0.375 X2 + (I - X / 2), Out2 untouched (a, b, c unused).  Returns 1 when taken, 0 when
// refused: every handle is then as it was.
int ntpoly_amd_isr_chain_step(const int* ih_X, const int* ih_X2, const int* order, const double* a, const double* b, const double* c,
                              int* ih_Out1, int* ih_Out2) {
  return ps_isr_chain_step(*get_unpacked(ih_X), *get_unpacked(ih_X2), *order, *a, *b, *c, *get_unpacked(ih_Out1), *get_unpacked(ih_Out2)) ? 1 : 0;
}
// DIAGNOSTIC surface, one rank: A is brought into slab form in a session of this call's own (a complex one where A is complex and
// FMA arithmetic, complex_tile and complex_sessions allow it), the transpose pass runs on it -- *conjugate != 0: the conjugate
// transpose -- and the PACKED result is installed in AT.  Returns 1, or 0 when gated or refused: AT is then as it was.  Does
// not depend on option slab_transpose
int ntpoly_amd_slab_transpose(const int* ih_A, int* ih_AT, const int* conjugate) {
  return ps_slab_transpose_step(*get<PSMatrix>(ih_A), *get<PSMatrix>(ih_AT), *conjugate != 0) ? 1 : 0;
}
// DIAGNOSTIC surface: one step of PowerBounds on one vector (option power_vector's kernels, whatever the option says) on the
// caller's x -- host arrays of N doubles, 2 N interleaved (re, im) for a complex A.  y = A x with every entry the chain over
// ascending k in the product's arithmetic, pruned as the product prunes (|y_i| > *threshold, else 0), NOT scaled; out = (sum conj(x)
// x, Re sum conj(x) y, sum |y|).  Returns 1 when the kernel ran, 0 when it was refused (process slices, a gather form that could
// not be built): y and out are then as they were.  Counts nothing
int ntpoly_amd_power_vector_step(const int* ih_A, const double* x, double* y, const double* threshold, double out[3]) {
  return ps_power_vector_diag(*get<PSMatrix>(ih_A), x, y, *threshold, out) ? 1 : 0;
}
// DIAGNOSTIC surface: one column dot pass of CGSolver's traces (option cg_dots: 1 for real operands, 2 for complex ones on one rank
// in FMA arithmetic) on caller-held U and V.  A session of its own for the operands' kind is opened, both operands are brought
// into slab form, k_cg_dots runs with one pair: diag_out[j] = the real part of entry (j, j) of MatrixMultiply(U^H, V, threshold) --
// the chain over ascending k of conj(U(k, j)) V(k, j) in the product's arithmetic, 0 where the product prunes it or has no entry --
// for the local columns, *trace_out = their sum in MatrixTrace's order over all ranks.  Operands that get no slab form (not
// run-like, an empty panel) go through the same chains on compressed columns, as in the loop.  Returns 1, or 0 when gated: both
// outputs are then as they were.  Counts nothing
int ntpoly_amd_cg_dots(const int* ih_U, const int* ih_V, double threshold, double* diag_out, double* trace_out) {
  return ps_cg_dots_diag(*get<PSMatrix>(ih_U), *get<PSMatrix>(ih_V), threshold, diag_out, trace_out) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end: one fused HPCP update on caller-held real matrices D1, DDH
// (what the loop's product D1 (I - D1) would be), D2DH (D1 DDH) and WH.  The operands are brought into slab form, the update runs,
// the outputs are packed into the result handles: D1out = (D1 + 2 D2DH) + (-2 sigma) DDH, DHout = I - D1out as CopyMatrix,
// IncrementMatrix(Identity, ., -1) and ScaleMatrix(., -1) build it, *energy = DotMatrix(D1out, WH).  Returns 1 when taken, 0 when
// refused: every handle and *energy are then as they were.
int ntpoly_amd_hpcp_update_step(const int* ih_D1, const int* ih_DDH, const int* ih_D2DH, const double* sigma, const int* ih_WH, int* ih_D1out,
                                int* ih_DHout, double* energy) {
  return ps_hpcp_update_step(*get_unpacked(ih_D1), *get_unpacked(ih_DDH), *get_unpacked(ih_D2DH), *sigma, *get_unpacked(ih_WH),
                             *get_unpacked(ih_D1out), *get_unpacked(ih_DHout), energy) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end: the fused trace pass of the HPCP loop on caller-held
// matrices, real (option hpcp_step) or complex (option complex_hpcp).  Both are brought into slab form where they are; out[0] =
// MatrixTrace(DDH), out[1] = MatrixTrace(D2DH) from one pass and one read-back.  Returns 1 when taken, 0 when refused or gated: out
// is then as it was.
int ntpoly_amd_hpcp_traces_step(const int* ih_DDH, const int* ih_D2DH, double out[2]) {
  return ps_hpcp_traces_step(*get_unpacked(ih_DDH), *get_unpacked(ih_D2DH), out) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end: one fused fold update on caller-held real matrices X, X2
// (what the loop's product X X would be) and WH.  The operands are brought into slab form, the pass runs, the new X is packed into
// the result handle: Xout = b X + a X2 as ScaleMatrix(X, b); IncrementMatrix(X2, X, a) at threshold 0 build it, *dot =
// DotMatrix(Xout, WH), *trace = MatrixTrace(Xout).  Returns 1 when taken, 0 when refused: every handle, *dot and *trace are then
// as they were.
int ntpoly_amd_scale_fold_update_step(const int* ih_X, const int* ih_X2, const double* a, const double* b, const int* ih_WH, int* ih_Xout,
                                      double* dot, double* trace) {
  return ps_saf_update_step(*get_unpacked(ih_X), *get_unpacked(ih_X2), *a, *b, *get_unpacked(ih_WH), *get_unpacked(ih_Xout), dot, trace) ? 1 : 0;
}
// ... and the pass of the scale branch: *dot = DotMatrix(X, WH) and *trace = MatrixTrace(X) of X as it stands, nothing written
int ntpoly_amd_scale_fold_dot_trace(const int* ih_X, const int* ih_WH, double* dot, double* trace) {
  return ps_saf_dot_trace_step(*get_unpacked(ih_X), *get_unpacked(ih_WH), dot, trace) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end, option wom_session = 2: the tail of one Heun trial of the WOM
// solvers on caller-held real matrices W, K0, K1 and RK1.  The operands are brought into slab form, the pass runs, RK2 is packed into
// the result handle: RK2out = (W + c K0) + c K1 with c = *step * 0.5 as CopyMatrix and two IncrementMatrix calls at *threshold build
// it, *err = MatrixNorm of RK1 - RK2 and *err2 = MatrixNorm of RK2 - W, each difference merged at *threshold.  Returns 1 when taken, 0
// when refused or gated: every handle, *err and *err2 are then as they were.
int ntpoly_amd_wom_heun_step(const int* ih_W, const int* ih_K0, const int* ih_K1, const int* ih_RK1, const double* step, const double* threshold,
                             int* ih_RK2out, double* err, double* err2) {
  return ps_wom_heun_step(*get_unpacked(ih_W), *get_unpacked(ih_K0), *get_unpacked(ih_K1), *get_unpacked(ih_RK1), *step, *threshold,
                          *get_unpacked(ih_RK2out), err, err2) ? 1 : 0;
}
// ... and the two dots of the canonical step: out[0] = DotMatrix(X, W), out[1] = DotMatrix(W, XA) from one kernel and one read-back,
// nothing written.  Returns 1 when taken, 0 when refused or gated: out is then as it was.
int ntpoly_amd_wom_c_dots(const int* ih_X, const int* ih_W, const int* ih_XA, double out[2]) {
  double d[2];
  if (!ps_wom_c_dots(*get_unpacked(ih_X), *get_unpacked(ih_W), *get_unpacked(ih_XA), d)) return 0;
  out[0] = d[0];
  out[1] = d[1];
  return 1;
}
// the hull of a column's four runs, in rows, up to which the Heun pass holds the column in registers (longer columns read their
// runs once per sweep): tests build operands on both sides of it
int ntpoly_amd_wom_heun_register_rows() { return slab_wom_heun_register_rows(); }
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end, option purify_session = 2: the tail of one iteration of
// PurificationExtrapolate on caller-held real matrices D (the working density), N (what the product D S D would be) and S (the
// overlap).  The operands are brought into slab form, the pass runs, N' is packed into the result handle: with *fold != 0 Nout = 2 D - N
// as ScaleMatrix(N, -1) and IncrementMatrix(D, N, 2) at threshold 0 build it, otherwise a copy of N; *norm = MatrixNorm of D - N'
// merged at threshold 0, *next_trace = DotMatrix(N', S).  One rank only.  Returns 1 when taken, 0 when refused or gated (several
// ranks are a gate): every handle, *norm and *next_trace are then as they were.
int ntpoly_amd_purify_tail_step(const int* ih_D, const int* ih_N, const int* ih_S, const int* fold, int* ih_Nout, double* norm,
                                double* next_trace) {
  return ps_purify_tail_step(*get_unpacked(ih_D), *get_unpacked(ih_N), *get_unpacked(ih_S), *fold != 0, *get_unpacked(ih_Nout), norm,
                             next_trace) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end, option poly_step = 2: the tail of a step of the real Chebyshev
// / Hermite recurrences on caller-held real matrices (engine.hpp ps_poly_step_diag).  TkOut = what IncrementMatrix(Tkm2, P, *a, 0)
// leaves in P, ROut = what IncrementMatrix(TkOut, R, *c, 0) then leaves in R.  The inputs are brought into slab form and keep their
// values, the pass runs, both outputs are packed into the result handles, which are none of the inputs and not one another.  One
// rank only.  Returns 1 when taken, 0 when refused or gated: every handle is then as it was.
int ntpoly_amd_poly_step(const int* ih_P, const int* ih_Tkm2, const int* ih_R, const double* a, const double* c, int* ih_TkOut, int* ih_ROut) {
  return ps_poly_step_diag(*get_unpacked(ih_P), *get_unpacked(ih_Tkm2), *get_unpacked(ih_R), *a, *c, *get_unpacked(ih_TkOut), *get_unpacked(ih_ROut)) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end, option sum_chain = 1: the scaled sum chain of the real solver
// loops on caller-held real matrices (engine.hpp ps_sum_chain_step).  Out = CopyMatrix(Base); ScaleMatrix(Out, *s);
// IncrementMatrix(A_k, Out, coeffs[k], threshold 0) for the *n_addends (1 .. 5) matrices whose handles ih_addends[k] point to;
// ScaleMatrix(Out, *post) -- *s == 1 and *post == 1 stand for no scaling call.  The inputs are brought into slab form and keep their
// values, the pass runs, the result is packed into Out, which is Base or none of the inputs.  One rank only.  Returns 1 when taken,
// 0 when refused or gated: every handle is then as it was.  Operands that are ALL complex: the same chain on (re, im) pairs with
// option complex_sum_chain = 2 in a session begun with complex_ok (FMA arithmetic, complex_tile, complex_sessions), counted in
// ntpoly_amd_complex_sum_chain_counts only; real and complex operands mixed are a gate.
int ntpoly_amd_sum_chain(const int* ih_Base, const double* s, const int* n_addends, const int* const* ih_addends, const double* coeffs,
                         const double* post, int* ih_Out) {
  if (*n_addends < 1 || *n_addends > 5) return 0;
  const PSMatrix* addends[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < *n_addends; ++k) addends[k] = get_unpacked(ih_addends[k]);
  return ps_sum_chain_step(*get_unpacked(ih_Base), *s, addends, coeffs, *n_addends, *post, *get_unpacked(ih_Out)) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end, option pade_session = 2: one of the two groups of merges of
// ComputeExponentialPade on caller-held real matrices.  For q = 1, 2  Out_q = CopyMatrix(Base); ScaleMatrix(Out_q, scales[q - 1]);
// IncrementMatrix(A_k, Out_q, coeffs[(q - 1) n_addends + k - 1], threshold 0) for k = 1 .. *n_addends; *n_addends is 1 (A2 and A3
// are not looked at) or 3.  The inputs are brought into slab form, the pass runs, both outputs are packed into the result handles.
// One rank only.  Returns 1 when taken, 0 when refused or gated (several ranks and any other *n_addends are gates): every handle is
// then as it was.
int ntpoly_amd_pade_chain_step(const int* ih_Base, const int* ih_A1, const int* ih_A2, const int* ih_A3, const int* n_addends, const double* scales,
                               const double* coeffs, int* ih_Out1, int* ih_Out2) {
  if (*n_addends != 1 && *n_addends != 3) return 0;
  const PSMatrix* addends[3] = {get_unpacked(ih_A1), nullptr, nullptr};
  if (*n_addends == 3) {
    addends[1] = get_unpacked(ih_A2);
    addends[2] = get_unpacked(ih_A3);
  }
  return ps_pade_chain_step(*get_unpacked(ih_Base), addends, *n_addends, scales, coeffs, *get_unpacked(ih_Out1), *get_unpacked(ih_Out2)) ? 1 : 0;
}
// DIAGNOSTIC surface, for use between ntpoly_amd_session_begin and _end: TRS4's chain on caller-held matrices X and X2 (what the
// loop's product X X would be), real or -- in a session with complex_ok and option complex_trs4 -- complex.  The two operands are
// brought into slab form, *trace_fx = dot(X2, 4 X - 3 X2) and *trace_gx = dot(X2, I - 2 X + X2) (their real parts) come from the
// first pass, P = (4 X - 3 X2) + sigma (I - 2 X + X2) from the second and is packed into the result handle.  Returns 1 when taken,
// 0 when refused or gated (sigma == 0 among the gates): every handle and both traces are then as they were.
int ntpoly_amd_trs4_chain_step(const int* ih_X, const int* ih_X2, const double* sigma, int* ih_P, double* trace_fx, double* trace_gx) {
  return ps_trs4_chain_step(*get_unpacked(ih_X), *get_unpacked(ih_X2), *sigma, *get_unpacked(ih_P), trace_fx, trace_gx) ? 1 : 0;
}
// ... and the energy pass of the complex loop: *energy = the real part of DotMatrix(X, WH) for a complex X, brought into slab form,
// and a complex WH as it stands (slab form, a read-only view or compressed columns), nothing written
int ntpoly_amd_trs4_energy(const int* ih_X, const int* ih_WH, double* energy) {
  return ps_trs4_energy_step(*get_unpacked(ih_X), *get_unpacked(ih_WH), energy) ? 1 : 0;
}
// the longest zero list an update of the fused PM loop has left on this rank since start (rows of one panel).  Not in
// counters.inc: it is the fifth slot of pm_session_counts(), a maximum, behind the four that ntpoly_amd_pm_session_counts gives
void ntpoly_amd_pm_session_longest_list(long long* out) { *out = pm_session_counts()[4]; }
// DIAGNOSTIC surface (one rank; matrices all real, or -- option complex_pm, FMA arithmetic, complex_tile, complex_sessions -- X, X2
// and X3 all complex: Out is then complex and Zout a pattern of stored (0, 0) entries; Z is read as a pattern, whatever its kind;
// mixed kinds, or complex operands with the option at 0, return 0): one sigma pass and one update of the PM loop's fused path on
// caller-held operands.  X: the iterate's non-zeros; Z: a matrix whose STORED PATTERN is the iterate's zero list (rows that compressed columns would hold
// as stored zeros; disjoint from X's pattern); X2, X3: what the loop's two products would be.  sc[0], sc[1] = trace and dot(., X)
// of X - X2 merged at thr; Out = the non-zeros of ScaleMatrix(X u Z, a1); IncrementMatrix(X2, ., a2, thr); IncrementMatrix(X3, ., a3,
// thr) and Zout = its stored zeros (as a pattern with zero values), both in compressed columns.  Returns 1 when taken, 0 when
// refused: nothing is written then.  The operands are left as they are either way.
int ntpoly_amd_pm_fused_step(const int* ih_X, const int* ih_Z, const int* ih_X2, const int* ih_X3, const double* a1, const double* a2,
                             const double* a3, const double* thr, int* ih_Out, int* ih_Zout, double* sc) {
  const PSMatrix &X = *get<PSMatrix>(ih_X), &Z = *get<PSMatrix>(ih_Z), &X2 = *get<PSMatrix>(ih_X2), &X3 = *get<PSMatrix>(ih_X3);
  PSMatrix &Out = *get<PSMatrix>(ih_Out), &Zout = *get<PSMatrix>(ih_Zout);
  CommScope cs(X.grid);
  if (world().active() || X.cplx != X2.cplx || X.cplx != X3.cplx || X.dim != Z.dim || X.dim != X2.dim || X.dim != X3.dim) return 0;
  const bool cplx = X.cplx;
  if (cplx ? (options().complex_pm == 0 || !complex_slab_loop(X)) : Z.cplx) return 0;
  DevMat x = X.loc.clone(), x2 = X2.loc.clone(), x3 = X3.loc.clone();
  // (complex: zero-free runs of (re, im) pairs, no read-only view)
  auto enter = [cplx](DevMat& m) { return cplx ? slab_enter_c(m, nullptr, false) : slab_enter(m); };
  if (!enter(x) || !enter(x2) || !enter(x3)) return 0;
  ZeroList zl, zn;
  zero_list_from_pattern(Z.loc, zl);
  DevMat R;
  double t[2] = {0.0, 0.0};
  if (cplx ? (!slab_pm_sigma_c(x, zl, x2, *thr, X.c0, t) || !slab_pm_update_c(x, zl, x2, x3, *a1, *a2, *a3, *thr, R, zn))
           : (!slab_pm_sigma(x, zl, x2, *thr, X.c0, t) || !slab_pm_update(x, zl, x2, x3, *a1, *a2, *a3, *thr, R, zn)))
    return 0;
  sc[0] = t[0];
  sc[1] = t[1];
  pack(R);
  for (PSMatrix* m : {&Out, &Zout}) { m->grid = X.grid; m->dim = X.dim; m->cplx = cplx; m->c0 = X.c0; m->c1 = X.c1; }
  Out.loc = std::move(R);
  Zout.loc = zero_list_matrix(zn, X.loc.rows, X.loc.cols, cplx);
  return 1;
}
// fused recurrence steps taken since start, by the Chebyshev / Hermite loops and by ntpoly_amd_recurrence_step (each is also
// counted as the two merges it replaces in ntpoly_amd_slab_algebra_counts; a declined step counts nothing here).  Not in
// counters.inc: one number by value, not an array
void ntpoly_amd_recurrence_step_count(long long* out) { *out = recurrence_step_count(); }
// (not in counters.inc: fields of the same struct and a fill ratio)
// block path of the last SpGEMM (spgemm_block.hip): out[0..2] = used, 16 x 16 x 16 tile products issued, candidate output
// super-tiles; fill = entries / (256 tiles) of the left operand
void ntpoly_amd_last_block_stats(long long* out, double* fill) {
  const SpgemmStats& s = last_spgemm_stats();
  out[0] = s.block; out[1] = s.block_tile_products; out[2] = s.block_cand;
  *fill = s.block_fill;
}
// tests: the block order the engine multiplies matrices of this dimension in (made from this matrix if there is none):
// position[index] (0-based; positions ascend along the order of the k steps); returns 1 on success
int ntpoly_amd_block_order(const int* ih, int* position) {
  PSMatrix& m = *get<PSMatrix>(ih);
  std::vector<int32_t> pos;
  if (!block_order_for(m.loc, pos)) return 0;
  std::memcpy(position, pos.data(), sizeof(int32_t) * pos.size());
  return 1;
}
void ntpoly_amd_drop_block_caches() { drop_block_caches(); }
// tests: the block order made FOR this matrix's pattern (spgemm_block.hip block_order_of_pattern -- what a solve in a block order
// across ranks redistributes its operands in; complex matrices from the moduli): position[index], *ns = super-blocks; 1 on success
int ntpoly_amd_block_order_of_pattern(const int* ih, int* position, int* ns) {
  PSMatrix& m = *get<PSMatrix>(ih);
  DevMat full = ps_gather_full(m);
  std::vector<int32_t> pos;
  int32_t s = 0;
  if (!block_order_of_pattern(full, pos, &s)) return 0;
  std::memcpy(position, pos.data(), sizeof(int32_t) * pos.size());
  *ns = s;
  return 1;
}
// (not in counters.inc: composed from a struct and the stream's own count)
// out[0] = halo exchanges of distributed multiplies so far, out[1] = host synchronisations inside them (counted where the
// host waits: sync_stream), out[2] = ALL host synchronisations of the process so far: a caller brackets a call with two
// reads to learn what the whole call cost (exchange, plan, totals)
void ntpoly_amd_exchange_stats(long long* out) {
  out[0] = exchange_stats().exchanges;
  out[1] = exchange_stats().host_syncs;
  out[2] = host_sync_count();
}
// tests: the bandwidth-reducing order of a (one-rank, real or complex) matrix' pattern; newpos[old] = new (0-based),
// returns 1 on success
int ntpoly_amd_band_order(const int* ih, int* newpos, long long* bandwidth) {
  PSMatrix& m = *get<PSMatrix>(ih);
  DevBuf<int32_t> pos;
  int64_t bw = 0;
  if (!find_band_order(m.loc, pos, &bw)) return 0;
  HIP_CHECK(hipMemcpyAsync(newpos, pos.p, sizeof(int32_t) * (size_t)m.loc.cols, hipMemcpyDeviceToHost, stream()));
  sync_stream();
  *bandwidth = bw;
  return 1;
}
// (not in counters.inc: a record of the last launch behind a count, read from a struct)
// what the last launch of the MFMA tile kernel chose (spgemm_tile.hpp TileLaunchInfo): out[0] = launches since the last
// ntpoly_amd_reset_spgemm_accum; of the last one out[1..8] = epi, waves per workgroup, rows per lane, label-aware, 32-bit
// offsets, source of the multiplier tile (0 prepared tiles, 1 runs through 64-bit pointers, 2 runs through the buffer per
// element, 3 runs as pairs of rows), largest k range of a block, tile-skip test carried
void ntpoly_amd_last_tile_launch(long long* out) {
  const TileLaunchInfo& t = last_tile_launch();
  out[0] = t.launches; out[1] = t.epi; out[2] = t.nw; out[3] = t.rows; out[4] = t.labelled; out[5] = t.off32;
  out[6] = t.bsrc; out[7] = t.max_kn; out[8] = t.skip;
}
// GatherMatrixToProcess (PSMatrixModule.F90:1704-1808, distributed_includes/GatherMatrixToProcess.f90, GatherMatrixToAll.f90):
// the whole distributed matrix as a LOCAL matrix (Matrix_lsr / Matrix_lsc of its scalar type) -- on every process
// (*within_slice_id < 0: the _all variants) or on the process with that rank inside its slice only (the _id variants: data
// stays replicated across slices; the other processes' ih_local is left as it was).  The callee constructs the handle.
void ntpoly_amd_gather_matrix_to_process(const int* ih_this, int* ih_local, const int* within_slice_id) {
  const PSMatrix& m = *get<PSMatrix>(ih_this);
  DevMat full = ps_gather_full(m);      // (collective: the panels travel to every rank; a process that is not the target drops them)
  const ProcessGrid& g = m.grid ? *m.grid : global_grid();
  const int slice_size = g.num_rows * g.num_cols;
  const int in_slice = g.global_rank - slice_size * g.my_slice;
  if (*within_slice_id >= 0 && *within_slice_id != in_slice) return;
  auto* L = new LocalMat();
  L->m = std::move(full);
  put(ih_local, L);
}
// CommSplitMatrix (PSMatrixModule.F90:1489-1541, distributed_includes/CommSplitMatrix.f90): a copy of the WHOLE matrix on each
// half of its process grid (SplitProcessGrid, ProcessGridModule.F90:430-515: along the slices where there are several, else
// along the longer of rows / columns).  The half lives on a sub-communicator (ncclCommSplit); every later call on the copy --
// products, reductions, solvers -- runs inside that half (engine.hpp CommScope).  One process: the copy itself, colour 0,
// "split along the slices" (the reference's base case, :11-14).
void ntpoly_amd_comm_split_matrix(const int* ih_this, int* ih_split, int* my_color, bool* split_slice) {
  const PSMatrix& m = *get<PSMatrix>(ih_this);
  if (!m.grid) NTP_FATAL("CommSplitMatrix of a matrix that was never constructed");
  auto* out = new PSMatrix();
  ps_comm_split(m, *out, my_color, split_slice);
  put(ih_split, out);
}
// SplitProcessGrid (ProcessGridModule.F90:430-515): the grid of this process's half (colour 0 / 1); collective over the old grid.
// The handle is owned by the engine (not to be handed to DestructProcessGrid_wrp); matrices constructed on it live on the
// half's communicator.  The reference's fifth result, the between-grid communicator, has no counterpart: what CommSplitMatrix
// uses it for is done by ntpoly_amd_comm_split_matrix.
void ntpoly_amd_split_process_grid(const int* ih_old_grid, int* ih_new_grid, int* my_color, bool* split_slice) {
  put(ih_new_grid, split_process_grid(*get<ProcessGrid>(ih_old_grid), my_color, split_slice));
}
// out[0] = rank of this process on the grid's communicator, out[1] = its size, out[2] = 1 when that is a sub-communicator
void ntpoly_amd_grid_comm_info(const int* ih_grid, int* out) {
  const ProcessGrid* g = get<ProcessGrid>(ih_grid);
  out[0] = g->global_rank;
  out[1] = g->total;
  out[2] = g->comm != nullptr ? 1 : 0;
}
// solves that ran in a BLOCK order across ranks (operands without runs or band: 3-D Hamiltonians), panel products of such
// solves that took the block path.  Not in counters.inc: composed from two sources
void ntpoly_amd_block_scope_counts(long long* out) {
  out[0] = band_scope_counts()[2];
  out[1] = block_scope_products();
}
// tests: the two vocabulary operations of the solver loops that have no entry point of their own in the reference's C ABI --
// IncrementMatrix(Identity, B, alpha) as the loops call it, and the norm of alpha A + beta B (returns 0 when the engine would
// form the difference instead)
void ntpoly_amd_increment_identity(const int* ih_identity, int* ih_matB, const double* alpha) {
  // (inside ntpoly_amd_session_begin / _end B stays as it is -- slab form included -- as in the solver loops that make this call)
  PSMatrix* B = (g_test_session && g_test_session->opened) ? get_unpacked(ih_matB) : get<PSMatrix>(ih_matB);
  ps_increment_identity(*get<PSMatrix>(ih_identity), *B, *alpha);
}
int ntpoly_amd_norm_axpby(const int* ih_matA, const int* ih_matB, const double* alpha, const double* beta, double* norm) {
  return ps_norm_axpby(*get<PSMatrix>(ih_matA), *get<PSMatrix>(ih_matB), *alpha, *beta, norm) ? 1 : 0;
}
// searches for a bandwidth-reducing order since start: one per sparsity pattern, not per operand (the next cycle of an
// SCF loop -- same pattern, other values -- reuses the order).  Not in counters.inc: one number by value, not an array
void ntpoly_amd_band_searches(long long* out) { *out = band_searches(); }
void ntpoly_amd_reset_spgemm_accum() {
  flush_spgemm_timers();
  spgemm_accum() = SpgemmAccum();
  tile_skip_counts()[0] = tile_skip_counts()[1] = 0;
  last_tile_launch().launches = 0;
}
// out: calls, products, nnz_c ; dout: alg_bytes, ms_numeric, ms_total
void ntpoly_amd_get_spgemm_accum(long long* out, double* dout) {
  flush_spgemm_timers();
  const SpgemmAccum& a = spgemm_accum();
  out[0] = a.calls; out[1] = a.products; out[2] = a.nnz_c;
  dout[0] = a.alg_bytes; dout[1] = a.ms_numeric; dout[2] = a.ms_total;
}
// per-iteration trace of the last solver call
int ntpoly_amd_trace_iterations() { return last_trace().iterations; }
void ntpoly_amd_trace_get(double* value, double* energy, double* sigma, long long* nnz) {
  const SolverTrace& t = last_trace();
  for (int i = 0; i < t.iterations; ++i) {
    value[i] = t.value[(size_t)i];
    energy[i] = t.energy[(size_t)i];
    sigma[i] = t.sigma[(size_t)i];
    nnz[i] = t.nnz[(size_t)i];
  }
}
void ntpoly_amd_trace_times(double* setup_ms, double* loop_ms) {
  *setup_ms = last_trace().setup_ms;
  *loop_ms = last_trace().loop_ms;
}
void ntpoly_amd_memory(long long* in_use, long long* cached) {
  *in_use = (long long)dev_bytes_in_use();
  *cached = (long long)dev_bytes_cached();
}
void ntpoly_amd_release_cache() {
  drop_operand_caches();
  dev_release_cache();
}
// hipMalloc calls the caching allocator had to make so far, and the host milliseconds they took
void ntpoly_amd_malloc_stats(long long* calls, double* ms) { dev_malloc_stats(calls, ms); }
// bulk triplet transfer (the reference ABI moves triplets one at a time)
void ntpoly_amd_triplets_set_r(int* ih_list, const long long* n, const int* col, const int* row, const double* val) {
  HostTriplets* t = get<HostTriplets>(ih_list);
  t->cplx = false;
  t->col.assign(col, col + *n);
  t->row.assign(row, row + *n);
  t->val.assign(val, val + *n);
}
void ntpoly_amd_triplets_set_c(int* ih_list, const long long* n, const int* col, const int* row, const double* val_ri) {
  HostTriplets* t = get<HostTriplets>(ih_list);
  t->cplx = true;
  t->col.assign(col, col + *n);
  t->row.assign(row, row + *n);
  t->val.assign(val_ri, val_ri + 2 * *n);
}
void ntpoly_amd_triplets_get(const int* ih_list, int* col, int* row, double* val) {
  const HostTriplets* t = get<HostTriplets>(ih_list);
  std::copy(t->col.begin(), t->col.end(), col);
  std::copy(t->row.begin(), t->row.end(), row);
  std::copy(t->val.begin(), t->val.end(), val);
}

// ===================================================================== ProcessGrid_c.h
void ConstructGlobalProcessGrid_wrp(const int* world_comm, const int* process_rows, const int* process_columns,
                                    const int* process_slices) {
  comm_bind_mpi(*world_comm);  // the reference's MPI communicator (ProcessGrid.cc:14): honoured when MPI is initialised
  construct_grid(global_grid(), *process_rows, *process_columns, *process_slices, base_world());
}
void ConstructGlobalProcessGrid_onlyslice_wrp(const int* world_comm, const int* process_slices) {
  comm_bind_mpi(*world_comm);
  construct_grid_default(global_grid(), *process_slices, base_world());
}
void ConstructGlobalProcessGrid_default_wrp(const int* world_comm) {
  comm_bind_mpi(*world_comm);
  construct_grid_default(global_grid(), 1, base_world());
}
void CopyProcessGrid_wrp(const int* ih_old_grid, int* ih_new_grid) {
  put(ih_new_grid, new ProcessGrid(*get<ProcessGrid>(ih_old_grid)));
}
int GetGlobalMySlice_wrp() { return global_grid().my_slice; }
int GetGlobalMyColumn_wrp() { return global_grid().my_col; }
int GetGlobalMyRow_wrp() { return global_grid().my_row; }
bool GetGlobalIsRoot_wrp() { return global_grid().is_root(); }
int GetGlobalNumSlices_wrp() { return global_grid().num_slices; }
int GetGlobalNumColumns_wrp() { return global_grid().num_cols; }
int GetGlobalNumRows_wrp() { return global_grid().num_rows; }
void WriteGlobalProcessGridInfo_wrp() { write_grid_info(global_grid()); }
void DestructGlobalProcessGrid_wrp() {}
void ConstructProcessGrid_wrp(int* ih_grid, const int* world_comm, const int* process_rows, const int* process_columns,
                              const int* process_slices) {
  comm_bind_mpi(*world_comm);
  ProcessGrid* g = new ProcessGrid();
  construct_grid(*g, *process_rows, *process_columns, *process_slices, base_world());
  put(ih_grid, g);
}
void ConstructProcessGrid_onlyslice_wrp(int* ih_grid, const int* world_comm, const int* process_slices) {
  comm_bind_mpi(*world_comm);
  ProcessGrid* g = new ProcessGrid();
  construct_grid_default(*g, *process_slices, base_world());
  put(ih_grid, g);
}
void ConstructProcessGrid_default_wrp(int* ih_grid, const int* world_comm) {
  comm_bind_mpi(*world_comm);
  ProcessGrid* g = new ProcessGrid();
  construct_grid_default(*g, 1, base_world());
  put(ih_grid, g);
}
int GetMySlice_wrp(const int* ih_grid) { return get<ProcessGrid>(ih_grid)->my_slice; }
int GetMyColumn_wrp(const int* ih_grid) { return get<ProcessGrid>(ih_grid)->my_col; }
int GetMyRow_wrp(const int* ih_grid) { return get<ProcessGrid>(ih_grid)->my_row; }
int GetNumSlices_wrp(const int* ih_grid) { return get<ProcessGrid>(ih_grid)->num_slices; }
int GetNumColumns_wrp(const int* ih_grid) { return get<ProcessGrid>(ih_grid)->num_cols; }
int GetNumRows_wrp(const int* ih_grid) { return get<ProcessGrid>(ih_grid)->num_rows; }
void WriteProcessGridInfo_wrp(const int* ih_grid) { write_grid_info(*get<ProcessGrid>(ih_grid)); }
void DestructProcessGrid_wrp(int* ih_grid) { delete get<ProcessGrid>(ih_grid); }

// ===================================================================== TripletList_c.h
void ConstructTripletList_r_wrp(int* ih_this, const int* size) {
  HostTriplets* t = new HostTriplets();
  t->cplx = false;
  t->col.assign((size_t)*size, 0);
  t->row.assign((size_t)*size, 0);
  t->val.assign((size_t)*size, 0.0);
  put(ih_this, t);
}
void ResizeTripletList_r_wrp(int* ih_this, const int* size) {
  HostTriplets* t = get<HostTriplets>(ih_this);
  t->col.resize((size_t)*size);
  t->row.resize((size_t)*size);
  t->val.resize((size_t)*size);
}
void AppendToTripletList_r_wrp(int* ih_this, const int* index_column, const int* index_row, const double* point_value) {
  HostTriplets* t = get<HostTriplets>(ih_this);
  t->col.push_back(*index_column);
  t->row.push_back(*index_row);
  t->val.push_back(*point_value);
}
void SetTripletAt_r_wrp(int* ih_this, const int* index, const int* index_column, const int* index_row,
                        const double* point_value) {
  HostTriplets* t = get<HostTriplets>(ih_this);
  const size_t i = (size_t)*index - 1;  // 1-based (TripletList.cc:44-48 adds 1)
  t->col[i] = *index_column;
  t->row[i] = *index_row;
  t->val[i] = *point_value;
}
void GetTripletAt_r_wrp(const int* ih_this, const int* index, int* index_column, int* index_row, double* point_value) {
  const HostTriplets* t = get<HostTriplets>(ih_this);
  const size_t i = (size_t)*index - 1;
  *index_column = t->col[i];
  *index_row = t->row[i];
  *point_value = t->val[i];
}
void DestructTripletList_r_wrp(int* ih_this) { delete get<HostTriplets>(ih_this); }
static void sort_triplets(const HostTriplets& in, HostTriplets& out) {
  const size_t n = in.size(), w = in.cplx ? 2 : 1;
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (in.col[a] != in.col[b]) return in.col[a] < in.col[b];
    return in.row[a] < in.row[b];
  });
  out.cplx = in.cplx;
  out.col.resize(n);
  out.row.resize(n);
  out.val.resize(n * w);
  for (size_t i = 0; i < n; ++i) {
    out.col[i] = in.col[order[i]];
    out.row[i] = in.row[order[i]];
    for (size_t k = 0; k < w; ++k) out.val[i * w + k] = in.val[order[i] * w + k];
  }
}
void SortTripletList_r_wrp(const int* ih_this, const int* matrix_size, int* h_sorted) {
  (void)matrix_size;
  HostTriplets* s = new HostTriplets();
  sort_triplets(*get<HostTriplets>(ih_this), *s);
  put(h_sorted, s);
}
int GetTripletListSize_r_wrp(const int* ih_this) { return (int)get<HostTriplets>(ih_this)->size(); }

void ConstructTripletList_c_wrp(int* ih_this, const int* size) {
  HostTriplets* t = new HostTriplets();
  t->cplx = true;
  t->col.assign((size_t)*size, 0);
  t->row.assign((size_t)*size, 0);
  t->val.assign((size_t)*size * 2, 0.0);
  put(ih_this, t);
}
void ResizeTripletList_c_wrp(int* ih_this, const int* size) {
  HostTriplets* t = get<HostTriplets>(ih_this);
  t->col.resize((size_t)*size);
  t->row.resize((size_t)*size);
  t->val.resize((size_t)*size * 2);
}
void AppendToTripletList_c_wrp(int* ih_this, const int* index_column, const int* index_row, const double* re,
                               const double* im) {
  HostTriplets* t = get<HostTriplets>(ih_this);
  t->col.push_back(*index_column);
  t->row.push_back(*index_row);
  t->val.push_back(*re);
  t->val.push_back(*im);
}
void SetTripletAt_c_wrp(int* ih_this, const int* index, const int* index_column, const int* index_row, const double* re,
                        const double* im) {
  HostTriplets* t = get<HostTriplets>(ih_this);
  const size_t i = (size_t)*index - 1;
  t->col[i] = *index_column;
  t->row[i] = *index_row;
  t->val[2 * i] = *re;
  t->val[2 * i + 1] = *im;
}
// the reference declares the outputs `const double*` (TripletList_c.h:26-28) but writes them
void GetTripletAt_c_wrp(const int* ih_this, const int* index, int* index_column, int* index_row, const double* re,
                        const double* im) {
  const HostTriplets* t = get<HostTriplets>(ih_this);
  const size_t i = (size_t)*index - 1;
  *index_column = t->col[i];
  *index_row = t->row[i];
  *const_cast<double*>(re) = t->val[2 * i];
  *const_cast<double*>(im) = t->val[2 * i + 1];
}
void DestructTripletList_c_wrp(int* ih_this) { delete get<HostTriplets>(ih_this); }
void SortTripletList_c_wrp(const int* ih_this, const int* matrix_size, int* h_sorted) {
  (void)matrix_size;
  HostTriplets* s = new HostTriplets();
  sort_triplets(*get<HostTriplets>(ih_this), *s);
  put(h_sorted, s);
}
int GetTripletListSize_c_wrp(const int* ih_this) { return (int)get<HostTriplets>(ih_this)->size(); }

// ===================================================================== Permutation_c.h
void ConstructDefaultPermutation_wrp(int* ih_this, const int* matrix_dimension) {
  Permutation* p = new Permutation();
  permutation_default(*p, *matrix_dimension);
  put(ih_this, p);
}
void ConstructReversePermutation_wrp(int* ih_this, const int* matrix_dimension) {
  Permutation* p = new Permutation();
  permutation_reverse(*p, *matrix_dimension);
  put(ih_this, p);
}
void ConstructRandomPermutation_wrp(int* ih_this, const int* matrix_dimension) {
  Permutation* p = new Permutation();
  permutation_random(*p, *matrix_dimension);
  put(ih_this, p);
}
void DestructPermutation_wrp(int* ih_this) { delete get<Permutation>(ih_this); }
// extension: explicit permutation (index_lookup, 1-based)
void ntpoly_amd_permutation_set(int* ih_this, const int* n, const int* index_lookup) {
  Permutation* p = get<Permutation>(ih_this);
  permutation_default(*p, *n);
  for (int i = 0; i < *n; ++i) p->index_lookup[(size_t)i] = index_lookup[i];
  for (int i = 0; i < *n; ++i) p->reverse_index_lookup[(size_t)p->index_lookup[(size_t)i] - 1] = i + 1;
}

// ===================================================================== memory pools
void ConstructMatrixMemoryPool_p_wrp(int* ih_this, const int* ih_matrix) {
  (void)ih_matrix;
  put(ih_this, new Pool());
}
void DestructMatrixMemoryPool_p_wrp(int* ih_this) { delete get<Pool>(ih_this); }
void ConstructMatrixMemoryPool_lr_wrp(int* ih_this, const int* columns, const int* rows) {
  (void)columns; (void)rows;
  put(ih_this, new Pool());
}
void DestructMatrixMemoryPool_lr_wrp(int* ih_this) { delete get<Pool>(ih_this); }
void ConstructMatrixMemoryPool_lc_wrp(int* ih_this, const int* columns, const int* rows) {
  (void)columns; (void)rows;
  put(ih_this, new Pool());
}
void DestructMatrixMemoryPool_lc_wrp(int* ih_this) { delete get<Pool>(ih_this); }

// ===================================================================== SolverParameters_c.h
void ConstructSolverParameters_wrp(int* ih_this) { put(ih_this, new SolverParameters()); }
void SetParametersConvergeDiff_wrp(int* ih_this, const double* v) { get<SolverParameters>(ih_this)->converge_diff = *v; }
void SetParametersMaxIterations_wrp(int* ih_this, const int* v) { get<SolverParameters>(ih_this)->max_iterations = *v; }
void SetParametersBeVerbose_wrp(int* ih_this, const bool* v) { get<SolverParameters>(ih_this)->be_verbose = *v; }
void SetParametersThreshold_wrp(int* ih_this, const double* v) { get<SolverParameters>(ih_this)->threshold = *v; }
void SetParametersLoadBalance_wrp(int* ih_this, const int* ih_permutation) {
  SolverParameters* p = get<SolverParameters>(ih_this);
  if (options().load_balance == 0) return;  // engine option: keep the caller's ordering (kernels.hpp)
  p->do_load_balancing = true;  // SolverParametersModule.F90:160-167
  p->balance_permutation = *get<Permutation>(ih_permutation);
}
void SetParametersStepThreshold_wrp(int* ih_this, const double* v) { get<SolverParameters>(ih_this)->step_thresh = *v; }
void SetParametersMonitorConvergence_wrp(int* ih_this, const bool* v) {
  get<SolverParameters>(ih_this)->monitor_convergence = *v;
}
void DestructSolverParameters_wrp(int* ih_this) { delete get<SolverParameters>(ih_this); }

// ===================================================================== Logging_c.h
void ActivateLogger_wrp(const bool* start_document) { log_activate(*start_document, nullptr); }
void ActivateLoggerFile_wrp(const bool* start_document, const char* file_name, const int* name_size) {
  log_activate(*start_document, fstring(file_name, name_size).c_str());
}
void DeactivateLogger_wrp() { log_deactivate(); }
// extension: the writing half of LoggingModule.F90 (WriteHeader / WriteElement / WriteListElement / Enter / ExitSubLog),
// which the reference exposes to Fortran callers only; used by the Fortran module layer (fortran/ntpoly_amd_modules.f90)
void ntpoly_amd_log_header(const char* text, const int* n) { log_header(fstring(text, n).c_str()); }
void ntpoly_amd_log_enter() { log_enter(); }
void ntpoly_amd_log_exit() { log_exit(); }
void ntpoly_amd_log_element_string(const char* key, const int* nk, const char* v, const int* nv) {
  log_element(fstring(key, nk).c_str(), fstring(v, nv).c_str());
}
void ntpoly_amd_log_element_int(const char* key, const int* nk, const int* v) { log_element(fstring(key, nk).c_str(), *v); }
void ntpoly_amd_log_element_real(const char* key, const int* nk, const double* v) { log_element(fstring(key, nk).c_str(), *v); }
void ntpoly_amd_log_element_bool(const char* key, const int* nk, const bool* v) { log_element(fstring(key, nk).c_str(), *v); }
void ntpoly_amd_log_list_element(const char* key, const int* nk) { log_list_element(fstring(key, nk).c_str()); }

// ===================================================================== PSMatrix_c.h
void ConstructEmptyMatrix_ps_wrp(int* ih_this, const int* matrix_dim) {
  PSMatrix* m = new PSMatrix();
  ps_construct_empty(*m, *matrix_dim, default_grid(), false);
  put(ih_this, m);
}
void ConstructEmptyMatrixPG_ps_wrp(int* ih_this, const int* matrix_dim, const int* ih_grid) {
  PSMatrix* m = new PSMatrix();
  ps_construct_empty(*m, *matrix_dim, get<ProcessGrid>(ih_grid), false);
  put(ih_this, m);
}
void CopyMatrix_ps_wrp(const int* ih_matA, int* ih_matB) {
  ApiSession ses(ih_matA);
  ps_copy(*ses.mat(ih_matA), *ses.mat(ih_matB));
}
void DestructMatrix_ps_wrp(int* ih_this) { delete get_unpacked(ih_this); }
void ConstructMatrixFromMatrixMarket_ps_wrp(int* ih_this, const char* file_name, const int* name_size) {
  PSMatrix* m = new PSMatrix();
  ps_read_matrix_market(*m, fstring(file_name, name_size), default_grid());
  put(ih_this, m);
}
void ConstructMatrixFromBinary_ps_wrp(int* ih_this, const char* file_name, const int* name_size) {
  PSMatrix* m = new PSMatrix();
  ps_read_binary(*m, fstring(file_name, name_size), default_grid());
  put(ih_this, m);
}
void ConstructMatrixFromMatrixMarketPG_ps_wrp(int* ih_this, const char* file_name, const int* name_size,
                                              const int* ih_grid) {
  PSMatrix* m = new PSMatrix();
  ps_read_matrix_market(*m, fstring(file_name, name_size), get<ProcessGrid>(ih_grid));
  put(ih_this, m);
}
void ConstructMatrixFromBinaryPG_ps_wrp(int* ih_this, const char* file_name, const int* name_size, const int* ih_grid) {
  PSMatrix* m = new PSMatrix();
  ps_read_binary(*m, fstring(file_name, name_size), get<ProcessGrid>(ih_grid));
  put(ih_this, m);
}
void WriteMatrixToBinary_ps_wrp(const int* ih_this, const char* file_name, const int* name_size) {
  ps_write_binary(*get<PSMatrix>(ih_this), fstring(file_name, name_size));
}
void WriteMatrixToMatrixMarket_ps_wrp(const int* ih_this, const char* file_name, const int* name_size) {
  ps_write_matrix_market(*get<PSMatrix>(ih_this), fstring(file_name, name_size));
}
void FillMatrixFromTripletList_psr_wrp(const int* ih_this, const int* ih_triplet_list) {
  PSMatrix* m = get<PSMatrix>(ih_this);
  if (m->cplx) {  // a real fill of a (so far) complex-typed handle makes it real, as the Fortran generic does
    m->cplx = false;
    m->loc.reset_empty(m->dim, m->c1 - m->c0, false);
  }
  ps_fill_from_triplets(*m, *get<HostTriplets>(ih_triplet_list));
}
void FillMatrixFromTripletList_psc_wrp(const int* ih_this, const int* ih_triplet_list) {
  PSMatrix* m = get<PSMatrix>(ih_this);
  if (!m->cplx) {  // FillMatrixFromTripletList_psc converts the matrix to complex (PSMatrixModule.F90:846-850)
    m->cplx = true;
    m->loc.reset_empty(m->dim, m->c1 - m->c0, true);
  }
  ps_fill_from_triplets(*m, *get<HostTriplets>(ih_triplet_list));
}
// extension: the Fortran API's prepartitioned_in = .TRUE. (PSMatrixModule.F90:796-825): every rank
// passes only entries of its own column panel, no exchange
void ntpoly_amd_fill_prepartitioned(const int* ih_this, const int* ih_triplet_list) {
  PSMatrix* m = get<PSMatrix>(ih_this);
  const HostTriplets* t = get<HostTriplets>(ih_triplet_list);
  if (m->cplx != t->cplx) {
    m->cplx = t->cplx;
  }
  m->loc = from_triplets(*t, m->dim, m->c1 - m->c0, m->c0);
}
void FillMatrixPermutation_ps_wrp(int* ih_this, const int* ih_permutation, const bool* permuterows) {
  ps_fill_permutation(*get<PSMatrix>(ih_this), get<Permutation>(ih_permutation)->index_lookup, *permuterows);
}
void FillMatrixIdentity_ps_wrp(int* ih_this) { ps_fill_identity(*get<PSMatrix>(ih_this)); }
void GetMatrixActualDimension_ps_wrp(const int* ih_this, int* size) { *size = get<PSMatrix>(ih_this)->dim; }
void GetMatrixLogicalDimension_ps_wrp(const int* ih_this, int* size) { *size = get<PSMatrix>(ih_this)->dim; }
void GetMatrixSize_ps_wrp(const int* ih_this, long int* size) { *size = (long int)ps_size(*get_unpacked(ih_this)); }   // (the entry count is kept in every storage form)
// PSMatrix_c.h:31 (wrapper PSMatrixModule_wrp.F90:259-266)
void FillMatrixDense_ps_wrp(int* ih_this) { ps_fill_dense(*get<PSMatrix>(ih_this)); }
// PSMatrix_c.h:37-44 (wrapper :344-391): blocks are [start, end) with 1-based indices, slices are inclusive
void GetMatrixBlock_psr_wrp(const int* ih_this, int* ih_triplet_list, int* start_row, int* end_row, int* start_column,
                            int* end_column) {
  const PSMatrix* m = get<PSMatrix>(ih_this);
  HostTriplets* t = get<HostTriplets>(ih_triplet_list);
  if (m->cplx) {
    PSMatrix r;
    ps_to_real(*m, r);
    ps_get_block(r, *start_row, *end_row, *start_column, *end_column, *t);
  } else {
    ps_get_block(*m, *start_row, *end_row, *start_column, *end_column, *t);
  }
}
void GetMatrixBlock_psc_wrp(const int* ih_this, int* ih_triplet_list, int* start_row, int* end_row, int* start_column,
                            int* end_column) {
  const PSMatrix* m = get<PSMatrix>(ih_this);
  HostTriplets* t = get<HostTriplets>(ih_triplet_list);
  if (!m->cplx) {
    PSMatrix c;
    ps_to_complex(*m, c);
    ps_get_block(c, *start_row, *end_row, *start_column, *end_column, *t);
  } else {
    ps_get_block(*m, *start_row, *end_row, *start_column, *end_column, *t);
  }
}
void GetMatrixSlice_wrp(const int* ih_this, int* ih_submatrix, int* start_row, int* end_row, int* start_column,
                        int* end_column) {
  ps_get_slice(*get<PSMatrix>(ih_this), *get<PSMatrix>(ih_submatrix), *start_row, *end_row, *start_column, *end_column);
}
// PSMatrix_c.h:48 (wrapper :417-425)
void ResizeMatrix_ps_wrp(int* ih_this, const int* new_size) { ps_resize(*get<PSMatrix>(ih_this), *new_size); }
// PSMatrix_c.h:67-68 (wrapper PSMatrixAlgebraModule_wrp.F90)
void MatrixDiagonalScale_psr_wrp(int* ih_mat, const int* ih_tlist) {
  ps_diagonal_scale(*get<PSMatrix>(ih_mat), *get<HostTriplets>(ih_tlist));
}
void MatrixDiagonalScale_psc_wrp(int* ih_mat, const int* ih_tlist) {
  PSMatrix* m = get<PSMatrix>(ih_mat);
  if (!m->cplx) {  // a complex diagonal turns the matrix complex, as ScaleMatrix_psc does (PSMatrixAlgebraModule.F90:486-504)
    PSMatrix c;
    ps_to_complex(*m, c);
    m->cplx = true;
    m->loc = std::move(c.loc);
  }
  ps_diagonal_scale(*m, *get<HostTriplets>(ih_tlist));
}
void GetMatrixTripletList_psr_wrp(const int* ih_this, int* ih_triplet_list) {
  const PSMatrix* m = get<PSMatrix>(ih_this);
  HostTriplets* t = get<HostTriplets>(ih_triplet_list);
  if (m->cplx) {  // ConvertMatrixToReal (PSMatrixModule.F90:1003-1004)
    PSMatrix r;
    ps_to_real(*m, r);
    ps_get_triplets(r, *t);
  } else {
    ps_get_triplets(*m, *t);
  }
}
void GetMatrixTripletList_psc_wrp(const int* ih_this, int* ih_triplet_list) {
  const PSMatrix* m = get<PSMatrix>(ih_this);
  HostTriplets* t = get<HostTriplets>(ih_triplet_list);
  if (!m->cplx) {
    PSMatrix c;
    ps_to_complex(*m, c);
    ps_get_triplets(c, *t);
  } else {
    ps_get_triplets(*m, *t);
  }
}
// (in a session of their own like the vocabulary calls above: a product of an earlier call that is still in slab form is transposed
// or conjugated there and stays there, option slab_transpose; a matrix in compressed columns is not converted for it)
void TransposeMatrix_ps_wrp(const int* ih_matA, int* ih_transmat) {
  if (options().slab_transpose == 0) { ps_transpose(*get<PSMatrix>(ih_matA), *get<PSMatrix>(ih_transmat)); return; }
  ApiSession ses(ih_matA);
  ps_transpose(*ses.mat(ih_matA), *ses.mat(ih_transmat));
}
void ConjugateMatrix_ps_wrp(int* ih_matA) {
  if (options().slab_transpose == 0) { ps_conjugate(*get<PSMatrix>(ih_matA)); return; }
  ApiSession ses(ih_matA);
  ps_conjugate(*ses.mat(ih_matA));
}
void GetMatrixProcessGrid_ps_wrp(const int* ih_this, int* ih_grid) {
  put(ih_grid, const_cast<ProcessGrid*>(get<PSMatrix>(ih_this)->grid));
}
int ntpoly_amd_matrix_is_complex(const int* ih_this) { return get<PSMatrix>(ih_this)->cplx ? 1 : 0; }
void ntpoly_amd_matrix_local_columns(const int* ih_this, int* c0, int* c1) {
  *c0 = get<PSMatrix>(ih_this)->c0;
  *c1 = get<PSMatrix>(ih_this)->c1;
}

void DotMatrix_psr_wrp(const int* ih_matA, const int* ih_matB, double* product) {
  double out[2];
  ApiSession ses(ih_matA);
  ps_dot(*ses.mat(ih_matA), *ses.mat(ih_matB), out);
  *product = out[0];
}
void DotMatrix_psc_wrp(const int* ih_matA, const int* ih_matB, double* product_real, double* product_imag) {
  double out[2];
  ApiSession ses(ih_matA);
  ps_dot(*ses.mat(ih_matA), *ses.mat(ih_matB), out);
  *product_real = out[0];
  *product_imag = out[1];
}
void IncrementMatrix_ps_wrp(const int* ih_matA, int* ih_matB, const double* alpha_in, const double* threshold_in) {
  ApiSession ses(ih_matA);
  ps_increment(*ses.mat(ih_matA), *ses.mat(ih_matB), *alpha_in, *threshold_in);
}
void MatrixPairwiseMultiply_ps_wrp(const int* ih_matA, const int* ih_matB, int* ih_matC) {
  ps_pairwise(*get<PSMatrix>(ih_matA), *get<PSMatrix>(ih_matB), *get<PSMatrix>(ih_matC));
}
void MatrixMultiply_ps_wrp(const int* ih_matA, const int* ih_matB, int* ih_matC, const double* alpha_in,
                           const double* beta_in, const double* threshold_in, int* ih_memory_pool_in) {
  (void)ih_memory_pool_in;
  ApiSession ses(ih_matA);
  ps_multiply(*ses.mat(ih_matA), *ses.mat(ih_matB), *ses.mat(ih_matC), *alpha_in, *beta_in, *threshold_in);
}
void ScaleMatrix_ps_wrp(int* ih_this, const double* constant) {
  ApiSession ses(ih_this);
  ps_scale(*ses.mat(ih_this), *constant);
}
double MatrixNorm_ps_wrp(const int* ih_this) {
  ApiSession ses(ih_this);
  return ps_norm(*ses.mat(ih_this));
}
double MeasureAsymmetry_ps_wrp(const int* ih_this) { return ps_measure_asymmetry(*get<PSMatrix>(ih_this)); }
void MatrixTrace_ps_wrp(const int* ih_this, double* trace_val) {
  ApiSession ses(ih_this);
  *trace_val = ps_trace(*ses.mat(ih_this));
}
int IsIdentity_ps_wrp(const int* ih_this) { return ps_is_identity(*get<PSMatrix>(ih_this)) ? 1 : 0; }
void SymmetrizeMatrix_ps_wrp(int* ih_this) { ps_symmetrize(*get<PSMatrix>(ih_this)); }

// ===================================================================== LoadBalancer_c.h, EigenBounds_c.h
void PermuteMatrix_wrp(const int* ih_mat_in, int* ih_mat_out, const int* ih_permutation, int* ih_memorypool) {
  (void)ih_memorypool;
  ps_permute(*get<PSMatrix>(ih_mat_in), *get<PSMatrix>(ih_mat_out), *get<Permutation>(ih_permutation), false);
}
void UndoPermuteMatrix_wrp(const int* ih_mat_in, int* ih_mat_out, const int* ih_permutation, int* ih_memorypool) {
  (void)ih_memorypool;
  ps_permute(*get<PSMatrix>(ih_mat_in), *get<PSMatrix>(ih_mat_out), *get<Permutation>(ih_permutation), true);
}
// EigenBounds_c.h:4-5 names the outputs (max_value, min_value) but the wrapper forwards them
// positionally to GershgorinBounds(this, min_value, max_value) (EigenBoundsModule_wrp.F90): first = min
void GershgorinBounds_wrp(const int* ih_Hamiltonian, double* max_value, double* min_value) {
  ps_gershgorin(*get<PSMatrix>(ih_Hamiltonian), max_value, min_value);
}

// ===================================================================== solvers
// outputs are declared `const double*` in DensityMatrixSolvers_c.h:4-23 but are written
// (DensityMatrixSolversModule_wrp.F90:57-58)
#define DENSITY_SOLVER(NAME, FN)                                                                              \
  void NAME(const int* ih_Hamiltonian, const int* ih_InverseSquareRoot, const double* trace, int* ih_Density, \
            const double* energy_value_out, const double* chemical_potential_out,                             \
            const int* ih_solver_parameters) {                                                                \
    FN(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_InverseSquareRoot), *trace, *get<PSMatrix>(ih_Density), \
       const_cast<double*>(energy_value_out), const_cast<double*>(chemical_potential_out),                    \
       *get<SolverParameters>(ih_solver_parameters));                                                         \
  }
DENSITY_SOLVER(PM_wrp, solver_pm)
DENSITY_SOLVER(TRS2_wrp, solver_trs2)
DENSITY_SOLVER(TRS4_wrp, solver_trs4)
DENSITY_SOLVER(HPCP_wrp, solver_hpcp)
// DensityMatrixSolvers_c.h:24-28 (wrapper DensityMatrixSolversModule_wrp.F90:129-153)
void ScaleAndFold_wrp(const int* ih_Hamiltonian, const int* ih_InverseSquareRoot, const double* trace, int* ih_Density,
                      const double* homo, const double* lumo, const double* energy_value_out,
                      const int* ih_solver_parameters) {
  solver_scale_and_fold(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_InverseSquareRoot), *trace,
                        *get<PSMatrix>(ih_Density), *homo, *lumo, const_cast<double*>(energy_value_out),
                        *get<SolverParameters>(ih_solver_parameters));
}
// DensityMatrixSolvers_c.h:34-38 (wrapper :183-231)
void EnergyDensityMatrix_wrp(const int* ih_Hamiltonian, const int* ih_Density, int* ih_EnergyDensity, const double* threshold) {
  energy_density_matrix(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_Density), *get<PSMatrix>(ih_EnergyDensity), *threshold);
}
void McWeenyStep_wrp(const int* ih_D, int* ih_DOut, const double* threshold) {
  mcweeny_step(*get<PSMatrix>(ih_D), *get<PSMatrix>(ih_DOut), nullptr, *threshold);
}
void McWeenyStepS_wrp(const int* ih_D, int* ih_DOut, const int* ih_S, const double* threshold) {
  mcweeny_step(*get<PSMatrix>(ih_D), *get<PSMatrix>(ih_DOut), get<PSMatrix>(ih_S), *threshold);
}
// The dense family of the reference (gather + LAPACK eigensolver, EigenSolversModule.F90:74-131): here the
// eigendecomposition runs on the GPU (two-sided Jacobi, solvers_extra.cpp, dense.hip); f(A) = V f(L) V^H.
void DenseDensity_wrp(const int* ih_Hamiltonian, const int* ih_InverseSquareRoot, const double* trace, int* ih_Density,
                      const double* energy_value_out, const double* chemical_potential_out, const int* ih_solver_parameters) {
  // DensityMatrixSolversModule.F90:1120-1160: the step-function occupation (no smearing)
  compute_dense_foe(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_InverseSquareRoot), *trace, *get<PSMatrix>(ih_Density),
                    nullptr, const_cast<double*>(energy_value_out), const_cast<double*>(chemical_potential_out),
                    *get<SolverParameters>(ih_solver_parameters));
}
static void dense_function(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters, const char* header,
                           double (*f)(double)) {
  const SolverParameters& p = *get<SolverParameters>(ih_solver_parameters);
  if (p.be_verbose && header) {
    log_header(header);
    log_enter();
  }
  dense_matrix_function(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), f, p);
  if (p.be_verbose && header) log_exit();
}
void DenseSquareRoot_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Square Root Solver", [](double v) { return std::sqrt(v); });
}
void DenseInverseSquareRoot_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Inverse Square Root Solver",
                 [](double v) { return 1.0 / std::sqrt(v); });
}
// FermiOperator_c.h:4-16 (FermiOperatorModule_wrp.F90): the wrapper always passes the inverse temperature
void ComputeDenseFOE_wrp(const int* ih_Hamiltonian, const int* ih_InverseSquareRoot, const double* trace, int* ih_Density,
                         const double* inv_temp_in, const double* energy_value_out, const double* chemical_potential_out,
                         const int* ih_solver_parameters) {
  compute_dense_foe(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_InverseSquareRoot), *trace, *get<PSMatrix>(ih_Density),
                    inv_temp_in, const_cast<double*>(energy_value_out), const_cast<double*>(chemical_potential_out),
                    *get<SolverParameters>(ih_solver_parameters));
}
void WOM_GC_wrp(const int* ih_Hamiltonian, const int* ih_InverseSquareRoot, int* ih_Density, const double* chemical_potential,
                const double* inv_temp, const double* energy_value_out, const int* ih_solver_parameters) {
  solver_wom(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_InverseSquareRoot), *get<PSMatrix>(ih_Density), *inv_temp,
             nullptr, chemical_potential, const_cast<double*>(energy_value_out), *get<SolverParameters>(ih_solver_parameters));
}
void WOM_C_wrp(const int* ih_Hamiltonian, const int* ih_InverseSquareRoot, int* ih_Density, const double* trace,
               const double* inv_temp, const double* energy_value_out, const int* ih_solver_parameters) {
  solver_wom(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_InverseSquareRoot), *get<PSMatrix>(ih_Density), *inv_temp,
             trace, nullptr, const_cast<double*>(energy_value_out), *get<SolverParameters>(ih_solver_parameters));
}
// EigenSolvers_c.h:4-15 -- positions as the Fortran wrapper binds them (EigenSolversModule_wrp.F90:19-62: matrix,
// eigenvalues, nvals, eigenvectors), which is how the C++ layer calls them (EigenSolvers.cc:12-21); the parameter
// NAMES in the C header are swapped
void EigenDecomposition_wrp(const int* ih_this, int* ih_eigenvalues, const int* nvals, int* ih_eigenvectors,
                            const int* ih_solver_parameters) {
  ps_eigendecomposition(*get<PSMatrix>(ih_this), *get<PSMatrix>(ih_eigenvalues), get<PSMatrix>(ih_eigenvectors), *nvals,
                        *get<SolverParameters>(ih_solver_parameters));
}
void EigenDecomposition_novec_wrp(const int* ih_this, int* ih_eigenvalues, const int* nvals, const int* ih_solver_parameters) {
  ps_eigendecomposition(*get<PSMatrix>(ih_this), *get<PSMatrix>(ih_eigenvalues), nullptr, *nvals,
                        *get<SolverParameters>(ih_solver_parameters));
}
void SingularValueDecompostion_wrp(const int* ih_this, int* ih_leftvectors, int* ih_rightvectors, int* ih_singularvalues,
                                   const int* ih_solver_parameters) {
  ps_svd(*get<PSMatrix>(ih_this), *get<PSMatrix>(ih_leftvectors), *get<PSMatrix>(ih_rightvectors),
         *get<PSMatrix>(ih_singularvalues), *get<SolverParameters>(ih_solver_parameters));
}
void EstimateGap_wrp(const int* ih_H, const int* ih_K, const double* chemical_potential, double* gap,
                     const int* ih_solver_parameters) {
  estimate_gap(*get<PSMatrix>(ih_H), *get<PSMatrix>(ih_K), *chemical_potential, gap, *get<SolverParameters>(ih_solver_parameters));
}
// LinearSolvers_c.h:4-7, Analysis_c.h:4-8
void CGSolver_wrp(const int* ih_MatA, int* ih_MatX, const int* ih_matB, const int* ih_solver_parameters) {
  solver_cg(*get<PSMatrix>(ih_MatA), *get<PSMatrix>(ih_MatX), *get<PSMatrix>(ih_matB), *get<SolverParameters>(ih_solver_parameters));
}
void CholeskyDecomposition_wrp(const int* ih_MatA, int* ih_MatL, const int* ih_solver_parameters) {
  ps_cholesky(*get<PSMatrix>(ih_MatA), *get<PSMatrix>(ih_MatL), -1, *get<SolverParameters>(ih_solver_parameters));
}
void PivotedCholeskyDecomposition_wrp(const int* ih_MatA, int* ih_MatL, const int* rank_in, const int* ih_solver_parameters) {
  ps_cholesky(*get<PSMatrix>(ih_MatA), *get<PSMatrix>(ih_MatL), *rank_in, *get<SolverParameters>(ih_solver_parameters));
}
void ReduceDimension_wrp(const int* ih_this, const int* dim, int* ih_reduced, const int* ih_solver_parameters) {
  reduce_dimension(*get<PSMatrix>(ih_this), *dim, *get<PSMatrix>(ih_reduced), *get<SolverParameters>(ih_solver_parameters));
}
// GeometryOptimization_c.h:4-10, MatrixConversion_c.h:4
void PurificationExtrapolate_wrp(const int* ih_PreviousDensity, const int* Overlap, const double* trace, int* ih_NewDensity,
                                 const int* ih_solver_parameters) {
  purification_extrapolate(*get<PSMatrix>(ih_PreviousDensity), *get<PSMatrix>(Overlap), *trace, *get<PSMatrix>(ih_NewDensity),
                           *get<SolverParameters>(ih_solver_parameters));
}
void LowdinExtrapolate_wrp(const int* ih_PreviousDensity, const int* OldOverlap, const int* NewOverlap, int* ih_NewDensity,
                           const int* ih_solver_parameters) {
  lowdin_extrapolate(*get<PSMatrix>(ih_PreviousDensity), *get<PSMatrix>(OldOverlap), *get<PSMatrix>(NewOverlap),
                     *get<PSMatrix>(ih_NewDensity), *get<SolverParameters>(ih_solver_parameters));
}
void SnapMatrixToSparsityPattern_wrp(int* ih_matA, const int* ih_matB) {
  snap_to_sparsity_pattern(*get<PSMatrix>(ih_matA), *get<PSMatrix>(ih_matB));
}

// ---- matrix polynomials: Polynomial_c.h:4-13, ChebyshevSolvers_c.h:4-15, HermiteSolvers_c.h:4-11
// (wrappers PolynomialSolversModule_wrp.F90:27-90, ChebyshevSolversModule_wrp.F90, HermiteSolversModule_wrp.F90).
// A polynomial handle holds `degree` coefficients; SetCoefficient takes a 1-based position (the C++ layer adds 1).
struct PolyHandle {
  std::vector<double> c;
};
static void poly_construct(int* ih_polynomial, int degree) {
  auto* h = new PolyHandle();
  h->c.assign((size_t)std::max(0, degree), 0.0);
  put(ih_polynomial, h);
}
static void poly_destruct(int* ih_polynomial) {
  delete get<PolyHandle>(ih_polynomial);
  std::memset(ih_polynomial, 0, sizeof(int) * SIZE_wrp);
}
static void poly_set(int* ih_polynomial, int degree, double coefficient) {
  PolyHandle* h = get<PolyHandle>(ih_polynomial);
  if (degree < 1 || degree > (int)h->c.size()) NTP_FATAL("SetCoefficient: degree out of range");
  h->c[(size_t)degree - 1] = coefficient;
}
void ConstructPolynomial_wrp(int* ih_polynomial, const int* degree) { poly_construct(ih_polynomial, *degree); }
void DestructPolynomial_wrp(int* ih_polynomial) { poly_destruct(ih_polynomial); }
void SetCoefficient_wrp(int* ih_polynomial, const int* degree, const double* coefficient) {
  poly_set(ih_polynomial, *degree, *coefficient);
}
void ConstructChebyshevPolynomial_wrp(int* ih_polynomial, const int* degree) { poly_construct(ih_polynomial, *degree); }
void DestructChebyshevPolynomial_wrp(int* ih_polynomial) { poly_destruct(ih_polynomial); }
void SetChebyshevCoefficient_wrp(int* ih_polynomial, const int* degree, const double* coefficient) {
  poly_set(ih_polynomial, *degree, *coefficient);
}
void ConstructHermitePolynomial_wrp(int* ih_polynomial, const int* degree) { poly_construct(ih_polynomial, *degree); }
void DestructHermitePolynomial_wrp(int* ih_polynomial) { poly_destruct(ih_polynomial); }
void SetHermiteCoefficient_wrp(int* ih_polynomial, const int* degree, const double* coefficient) {
  poly_set(ih_polynomial, *degree, *coefficient);
}
void HornerCompute_wrp(const int* ih_InputMat, int* ih_OutputMat, const int* ih_polynomial, const int* ih_solver_parameters) {
  polynomial_horner(*get<PSMatrix>(ih_InputMat), *get<PSMatrix>(ih_OutputMat), get<PolyHandle>(ih_polynomial)->c,
     *get<SolverParameters>(ih_solver_parameters));
}
void PatersonStockmeyerCompute_wrp(const int* ih_InputMat, int* ih_OutputMat, const int* ih_polynomial, const int* ih_solver_parameters) {
  polynomial_paterson_stockmeyer(*get<PSMatrix>(ih_InputMat), *get<PSMatrix>(ih_OutputMat), get<PolyHandle>(ih_polynomial)->c,
     *get<SolverParameters>(ih_solver_parameters));
}
void ChebyshevCompute_wrp(const int* ih_InputMat, int* ih_OutputMat, const int* ih_polynomial, const int* ih_solver_parameters) {
  chebyshev_compute(*get<PSMatrix>(ih_InputMat), *get<PSMatrix>(ih_OutputMat), get<PolyHandle>(ih_polynomial)->c,
     *get<SolverParameters>(ih_solver_parameters));
}
void FactorizedChebyshevCompute_wrp(const int* ih_InputMat, int* ih_OutputMat, const int* ih_polynomial, const int* ih_solver_parameters) {
  chebyshev_factorized(*get<PSMatrix>(ih_InputMat), *get<PSMatrix>(ih_OutputMat), get<PolyHandle>(ih_polynomial)->c,
     *get<SolverParameters>(ih_solver_parameters));
}
void HermiteCompute_wrp(const int* ih_InputMat, int* ih_OutputMat, const int* ih_polynomial, const int* ih_solver_parameters) {
  hermite_compute(*get<PSMatrix>(ih_InputMat), *get<PSMatrix>(ih_OutputMat), get<PolyHandle>(ih_polynomial)->c,
     *get<SolverParameters>(ih_solver_parameters));
}

// ---- matrix functions: ExponentialSolvers_c.h, TrigonometrySolvers_c.h, RootSolvers_c.h, EigenBounds_c.h
void ComputeExponential_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  compute_exponential(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters));
}
void ComputeLogarithm_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  compute_logarithm(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters));
}
void Sine_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  compute_sine(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters));
}
void Cosine_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  compute_cosine(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters));
}
void ComputeRoot_wrp(const int* ih_inputmat, int* ih_outputmat, const int* root, const int* ih_solver_parameters) {
  compute_root(*get<PSMatrix>(ih_inputmat), *get<PSMatrix>(ih_outputmat), *root, *get<SolverParameters>(ih_solver_parameters));
}
void ComputeInverseRoot_wrp(const int* ih_inputmat, int* ih_outputmat, const int* root, const int* ih_solver_parameters) {
  compute_inverse_root(*get<PSMatrix>(ih_inputmat), *get<PSMatrix>(ih_outputmat), *root,
                       *get<SolverParameters>(ih_solver_parameters));
}
void PowerBounds_wrp(const int* ih_Hamiltonian, double* max_value, const int* ih_solver_parameters) {
  power_bounds(*get<PSMatrix>(ih_Hamiltonian), max_value, *get<SolverParameters>(ih_solver_parameters), false);
}
// dense (eigendecomposition) variants: ExponentialSolversModule.F90:372-404,637-669, TrigonometrySolversModule.F90:66-150,
// InverseSolversModule.F90:152-181, SignSolversModule.F90:67-96
void ComputeExponentialPade_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  compute_exponential_pade(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters));
}
void ComputeDenseExponential_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Exponential Solver", [](double v) { return std::exp(v); });
}
void ComputeDenseLogarithm_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Logarithm Solver", [](double v) { return std::log(v); });
}
void DenseSine_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Trigonometry Solver", [](double v) { return std::sin(v); });
}
void DenseCosine_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Trigonometry Solver", [](double v) { return std::cos(v); });
}
void DenseInvert_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Inverse Solver", [](double v) { return 1.0 / v; });
}
void DenseSignFunction_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  dense_function(ih_Input, ih_Output, ih_solver_parameters, "Sign Function Solver", [](double v) { return v < 0.0 ? -1.0 : 1.0; });
}

void SignFunction_wrp(const int* ih_mat1, int* ih_signmat, const int* ih_solver_parameters) {
  solver_sign(*get<PSMatrix>(ih_mat1), *get<PSMatrix>(ih_signmat), *get<SolverParameters>(ih_solver_parameters));
}
void PolarDecomposition_wrp(const int* ih_mat1, int* ih_umat, int* ih_hmat, const int* ih_solver_parameters) {
  solver_polar(*get<PSMatrix>(ih_mat1), *get<PSMatrix>(ih_umat), get<PSMatrix>(ih_hmat),
               *get<SolverParameters>(ih_solver_parameters));
}
void Invert_wrp(const int* ih_Hamiltonian, int* ih_Inverse, const int* ih_solver_parameters) {
  solver_invert(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_Inverse), *get<SolverParameters>(ih_solver_parameters));
}
void PseudoInverse_wrp(const int* ih_Hamiltonian, int* ih_Inverse, const int* ih_solver_parameters) {
  solver_pseudoinverse(*get<PSMatrix>(ih_Hamiltonian), *get<PSMatrix>(ih_Inverse),
                       *get<SolverParameters>(ih_solver_parameters));
}
void SquareRoot_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  solver_square_root(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters),
                     false, 5);
}
void InverseSquareRoot_wrp(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters) {
  solver_square_root(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters),
                     true, 5);
}
// extension: one TRS2 iteration on caller-held matrices (what TRS2_wrp runs inside its loop); lets a
// driver time exactly K iterations.  X and X2 must be constructed; returns energy and sigma.
// trace_io: in = trace(X) when the caller has it from the previous step (NaN: computed here), out = trace of the new X
// (accumulated in the pass that evaluates the energy), exactly what the solver loop hands from iteration to iteration.
void ntpoly_amd_trs2_step(int* ih_X, int* ih_X2, const int* ih_WH, const double* trace, const double* threshold,
                          double* energy_out, double* sigma_out, double* trace_io) {
  *energy_out = trs2_step(*get_unpacked(ih_X), *get<PSMatrix>(ih_X2), *get<PSMatrix>(ih_WH), *trace, *threshold, sigma_out,
                          trace_io);
}
// extension: the reference's optional order_in argument (SquareRootSolversModule.F90:30-61) is not
// reachable through its C ABI; expose it for tests
void ntpoly_amd_square_root_order(const int* ih_Input, int* ih_Output, const int* ih_solver_parameters,
                                  const int* inverse, const int* order) {
  solver_square_root(*get<PSMatrix>(ih_Input), *get<PSMatrix>(ih_Output), *get<SolverParameters>(ih_solver_parameters),
                     *inverse != 0, *order);
}

// ===================================================================== SMatrix_c.h (local matrices, config 2)
#define LOCAL_API(SUF, CPLX)                                                                                     \
  void ConstructMatrixFromTripletList_##SUF##_wrp(int* ih_this, const int* ih_triplet_list, const int* rows,     \
                                                  const int* columns) {                                          \
    ensure_init();                                                                                               \
    LocalMat* m = new LocalMat();                                                                                \
    m->m = from_triplets(*get<HostTriplets>(ih_triplet_list), *rows, *columns, 0);                               \
    put(ih_this, m);                                                                                             \
  }                                                                                                              \
  void ConstructZeroMatrix_##SUF##_wrp(int* ih_this, const int* rows, const int* columns) {                      \
    ensure_init();                                                                                               \
    LocalMat* m = new LocalMat();                                                                                \
    m->m.reset_empty(*rows, *columns, CPLX);                                                                     \
    put(ih_this, m);                                                                                             \
  }                                                                                                              \
  void ConstructMatrixFromFile_##SUF##_wrp(int* ih_this, const char* file_name, const int* name_size) {          \
    ensure_init();                                                                                               \
    LocalMat* m = new LocalMat();                                                                                \
    int rows = 0, cols = 0;                                                                                      \
    HostTriplets t;                                                                                              \
    read_matrix_market_file(fstring(file_name, name_size), t, &rows, &cols, CPLX);                               \
    m->m = from_triplets(t, rows, cols, 0);                                                                      \
    put(ih_this, m);                                                                                             \
  }                                                                                                              \
  void DestructMatrix_##SUF##_wrp(int* ih_this) { delete get<LocalMat>(ih_this); }                               \
  void CopyMatrix_##SUF##_wrp(const int* ih_matA, int* ih_matB) {                                                \
    get<LocalMat>(ih_matB)->m = get<LocalMat>(ih_matA)->m.clone();                                               \
  }                                                                                                              \
  void GetMatrixRows_##SUF##_wrp(const int* ih_this, int* rows) { *rows = get<LocalMat>(ih_this)->m.rows; }      \
  void GetMatrixColumns_##SUF##_wrp(const int* ih_this, int* columns) { *columns = get<LocalMat>(ih_this)->m.cols; } \
  void ScaleMatrix_##SUF##_wrp(int* ih_this, const double* constant) { scale(get<LocalMat>(ih_this)->m, *constant); } \
  void IncrementMatrix_##SUF##_wrp(const int* ih_matA, int* ih_matB, const double* alpha_in,                     \
                                   const double* threshold_in) {                                                 \
    increment(get<LocalMat>(ih_matA)->m, get<LocalMat>(ih_matB)->m, *alpha_in, *threshold_in);                   \
  }                                                                                                              \
  void PairwiseMultiplyMatrix_##SUF##_wrp(const int* ih_matA, const int* ih_matB, int* ih_matC) {                \
    pairwise(get<LocalMat>(ih_matA)->m, get<LocalMat>(ih_matB)->m, get<LocalMat>(ih_matC)->m, false);            \
  }                                                                                                              \
  void TransposeMatrix_##SUF##_wrp(const int* ih_matA, int* ih_matAT) {                                          \
    get<LocalMat>(ih_matAT)->m = transpose(get<LocalMat>(ih_matA)->m);                                           \
  }                                                                                                              \
  void MatrixToTripletList_##SUF##_wrp(const int* ih_this, int* ih_triplet_list) {                               \
    to_triplets(get<LocalMat>(ih_this)->m, 0, *get<HostTriplets>(ih_triplet_list));                              \
  }                                                                                                              \
  /* ExtractMatrixRow.f90 / ExtractMatrixColumn.f90 (1-based number), MatrixDiagonalScale (column col *= value), */ \
  /* PrintMatrix.f90 (MatrixMarket text to stdout or a file) */                                                  \
  void ExtractMatrixColumn_##SUF##_wrp(const int* ih_this, int* column_number, int* ih_column_out) {             \
    get<LocalMat>(ih_column_out)->m = column_slice(get<LocalMat>(ih_this)->m, *column_number - 1, *column_number); \
  }                                                                                                              \
  void ExtractMatrixRow_##SUF##_wrp(const int* ih_this, int* row_number, int* ih_row_out) {                      \
    DevMat t = transpose(get<LocalMat>(ih_this)->m);                                                             \
    DevMat c = column_slice(t, *row_number - 1, *row_number);                                                    \
    get<LocalMat>(ih_row_out)->m = transpose(c);                                                                 \
  }                                                                                                              \
  void MatrixDiagonalScale_##SUF##_wrp(int* ih_mat, const int* ih_tlist) {                                       \
    local_diagonal_scale(get<LocalMat>(ih_mat)->m, *get<HostTriplets>(ih_tlist));                                \
  }                                                                                                              \
  void PrintMatrix_##SUF##_wrp(const int* ih_this) { local_print(get<LocalMat>(ih_this)->m, nullptr); }          \
  void PrintMatrixF_##SUF##_wrp(const int* ih_this, const char* file_name, const int* name_size) {                \
    const std::string path = fstring(file_name, name_size);                                                      \
    local_print(get<LocalMat>(ih_this)->m, path.c_str());                                                        \
  }                                                                                                              \
  /* GemmMatrix (sparse_includes/GemmMatrix.f90:1-101) */                                                        \
  void MatrixMultiply_##SUF##_wrp(const int* ih_matA, const int* ih_matB, int* ih_matC, const bool* IsATransposed, \
                                  const bool* IsBTransposed, const double* alpha, const double* beta,            \
                                  const double* threshold, int* ih_matrix_memory_pool) {                         \
    (void)ih_matrix_memory_pool;                                                                                 \
    const DevMat& A0 = get<LocalMat>(ih_matA)->m;                                                                \
    const DevMat& B0 = get<LocalMat>(ih_matB)->m;                                                                \
    DevMat& C = get<LocalMat>(ih_matC)->m;                                                                       \
    const double sa = (double)A0.nnz / ((double)A0.rows * (double)A0.cols);                                      \
    const double sb = (double)B0.nnz / ((double)B0.rows * (double)B0.cols);                                      \
    const bool dense_rule = std::min(sa, sb) > 0.1;                                                              \
    DevMat At, Bt;                                                                                               \
    if (*IsATransposed) At = transpose(A0);                                                                      \
    if (*IsBTransposed) Bt = transpose(B0);                                                                      \
    DevMat AB;                                                                                                   \
    spgemm(*IsATransposed ? At : A0, *IsBTransposed ? Bt : B0, AB, *alpha, *threshold, dense_rule);              \
    if (std::fabs(*beta) > 0 && C.rows == AB.rows && C.cols == AB.cols) {                                        \
      scale(C, *beta);                                                                                           \
      increment(AB, C, 1.0, 0.0);                                                                                \
    } else {                                                                                                     \
      C = std::move(AB);                                                                                         \
    }                                                                                                            \
  }

LOCAL_API(lsr, false)
LOCAL_API(lsc, true)

void DotMatrix_lsr_wrp(const int* ih_matA, const int* ih_matB, double* product) {
  double out[2];
  dot(get<LocalMat>(ih_matA)->m, get<LocalMat>(ih_matB)->m, out);
  *product = out[0];
}
void DotMatrix_lsc_wrp(const int* ih_matA, const int* ih_matB, double* product_real, double* product_complex) {
  double out[2];
  dot(get<LocalMat>(ih_matA)->m, get<LocalMat>(ih_matB)->m, out);
  *product_real = out[0];
  *product_complex = out[1];
}
void ConjugateMatrix_lsc_wrp(int* ih_matA) { conjugate(get<LocalMat>(ih_matA)->m); }

}  // extern "C"
