// Launchers of the hand-written gfx950 kernels (kernels.hip).  Everything operates on
// device-resident column-compressed matrices (DevMat) on ctx().stream.
#pragma once
#include <functional>
#include "common.hpp"

namespace ntp {

// Per-call statistics of the SpGEMM (for bench.py's roofline accounting).
struct SpgemmStats {
  int64_t nnz_a = 0, nnz_b = 0, nnz_c = 0;
  int64_t products = 0;        // intermediate products IP = sum_j sum_{k in B(:,j)} nnz(A(:,k)); on the register-slab path
                               // only counted when the time_kernels option is on (it costs a gather per entry of B)
  int64_t tmp_entries = 0;     // upper-bound entries reserved for the numeric pass
  int slab = 0;                // 1 when the register-slab kernel computed the product
  int fused = 0;               // 1 / 2: with the fused epilogue of a purification step (SlabFusion::mode)
  int64_t bin_cols[6] = {0, 0, 0, 0, 0, 0};
  int64_t overflow_cols = 0;   // columns that left the LDS hash for the HBM accumulator
  // grouped LDS-hash path (spgemm_grouped.hip): 1 when it computed the product; columns handed back to the per-column
  // kernels, table class reached, min-hash clustering used, union ratio (1 = the columns of a group are identical)
  int grouped = 0;
  int strips = 0;              // > 0: the product was computed in that many row strips of A (columns with too many distinct rows for
                               // the grouped kernel's tables: kernels.hip spgemm_striped)
  int64_t gh_failed_cols = 0, gh_groups = 0, gh_tile_rows = 0;
  int gh_level = 0, gh_minhash = 0;
  double gh_union_ratio = 0;
  // block path (spgemm_block.hip): 1 when it computed the product; tile fill of A, 16 x 16 x 16 tile products issued
  // (4 matrix instructions each), candidate output super-tiles
  int block = 0;
  double block_fill = 0;
  int64_t block_tile_products = 0, block_cand = 0;
  int thin = 0;                // 1: the thin-left kernel (spgemm_thin.hip) computed the product
  float ms_total = 0.f;        // filled only when timing is enabled
  float ms_numeric = 0.f;
};

// the option table (options.inc, where every option is documented) as plain int fields ...
struct EngineOptions {
#define NTP_OPTION(name, dflt, env) int name = dflt;
#include "options.inc"
#undef NTP_OPTION
};
// ... and as the one array that set, get and the environment walk go through (has_env: NTPOLY_AMD_<NAME> sets the field at start)
struct OptionEntry {
  const char* name;
  int EngineOptions::*field;
  bool has_env;
};
constexpr OptionEntry option_table[] = {   // (internal linkage: the library exports no symbol for it)
#define NTP_OPTION_ENV true
#define NTP_OPTION_NOENV false
#define NTP_OPTION(name, dflt, env) {#name, &EngineOptions::name, NTP_OPTION_##env},
#include "options.inc"
#undef NTP_OPTION
#undef NTP_OPTION_ENV
#undef NTP_OPTION_NOENV
};
// read once, at the first call: the table's defaults, then the environment
EngineOptions& options();
SpgemmStats& last_spgemm_stats();
// accumulated since reset: number of calls, products, algorithmic bytes, numeric-kernel ms
struct SpgemmAccum { int64_t calls = 0, products = 0, nnz_c = 0; double alg_bytes = 0, ms_numeric = 0, ms_total = 0; };
SpgemmAccum& spgemm_accum();
// resolve the HIP events recorded by the timed multiplies since the last call (time_kernels option)
void flush_spgemm_timers();

// A product left "loose": every column sits in the upper-bound slot the numeric kernel wrote it to (entries
// start[j] .. start[j] + count[j]), the compaction pass has not run.  Produced by spgemm(..., &loose) on the
// register-slab path and consumed by axpby(loose, ...): the TRS2 update reads X*X straight from the slots.
struct LooseProduct {
  bool valid = false;
  int32_t rows = 0, cols = 0;
  int64_t slots = 0;            // capacity of inner / val (= start[cols])
  DevBuf<int64_t> start;        // cols + 1
  DevBuf<int32_t> count;        // cols
  DevBuf<int32_t> inner;
  DevBuf<double> val;           // real only
  DevBuf<int64_t> prod_scan;    // statistics: [prod_index] = product count of the multiply (when counted)
  int64_t prod_index = -1;
};

// C = alpha * A * B with NTPoly's prune rule.  A: (m x k), B: (k x n), same scalar type.
// dense_rule = the reference's dense-branch order (threshold before alpha, DenseBranch.f90:14-15).
// loose != nullptr: if the register-slab kernel computes the product, leave it uncompacted in *loose (loose->valid,
// C untouched); otherwise C is produced as usual and loose->valid stays false.
// arange: the columns [a, b) of A that the rows of B can name, when the caller knows them (gathered operands are
// dim wide but populated over the halo range only): the per-column planning work then covers that range only
struct ColRange { int32_t a, b; };
// A purification step computed inside the register-slab kernel (A = B = X, real, one rank): the product never exists as
// a matrix.  mode 1: result = X * X; mode 2: result = am * (X * X) + bm * X, merged by the AddSparseVectors rules with
// `threshold`.  Either way dot = sum result .* D and trace = trace(result) come out of the same kernel and the result
// is left LOOSE (no compaction).  done = false on return: the multiply took another path, or the kernel met a case it
// does not decide (SlabFuseArgs in kernels.hip) -- the product was then computed the ordinary way (C / *loose).
struct SlabFusion {
  int mode = 0;
  double am = 0, bm = 0, threshold = 0;
  const DevMat* D = nullptr;
  int32_t col_offset = 0;
  int32_t panel_c0 = -1;      // >= 0: B is the column panel [panel_c0, panel_c0 + cols) of the iterate, A holds those columns
  bool done = false;
  DevMat result;
  double dot = 0, trace = 0;
  int64_t product_nnz = 0;
  int64_t refused = 0;
};
void spgemm(const DevMat& A, const DevMat& B, DevMat& C, double alpha, double threshold,
            bool dense_rule, LooseProduct* loose = nullptr, const ColRange* arange = nullptr, SlabFusion* fuse = nullptr);
// while one is alive, a product that the block path computes (spgemm_block.hip) is left in block form (DevMat::blk): for
// callers that hand it on to another product or pack() it themselves
// One TRS2 step with the iterate in block form (X: compressed columns of a dimension the block path multiplies, or block
// form; left in block form): mode 1: X <- X X, mode 2: X <- 2 X - X X by the AddSparseVectors rules; out[0] = dot(X, D),
// out[2] = trace(X).  false: not taken, X unchanged.
bool trs2_block_step(DevMat& X, int mode, double threshold, bool dense_rule, const DevMat& D, double out[4]);
struct BlockKeepScope {
  BlockKeepScope();
  ~BlockKeepScope();
  BlockKeepScope(const BlockKeepScope&) = delete;
  BlockKeepScope& operator=(const BlockKeepScope&) = delete;
};
// the same step on an iterate already in slab form (DevMat::slab, written by a previous fused step): X is replaced by
// the result (again in slab form).  false: not taken (X unchanged; pack() it and use spgemm)
struct SlabReduce {   // panel steps: the sum over the ranks rides on the step's own read-back
  void (*allreduce)(double* dev4) = nullptr;   // enqueues an all-reduce (sum) of 4 doubles on the engine stream
  double reduced[4] = {0, 0, 0, 0};            // (dot, 0, trace, number of ranks whose kernel succeeded)
  bool done = false;                           // the collective was entered (false: the step gave up before its kernel)
};
struct SlabHalo {   // A side of a panel step: the columns ka .. kb (global numbers) of the distributed iterate
  int32_t ka = 0, kb = 0;
  const int32_t* first = nullptr;            // [kb - ka] device: extents of column ka + i
  const int32_t* last = nullptr;
  const unsigned long long* addr = nullptr;  // [kb - ka] device: address of its run (own buffer or receive buffer)
  const int32_t* count = nullptr;            // [kb - ka] device, optional (statistics): entries of the column
  int row_pad = 1;                           // the received runs sit in slots aligned to this many rows, zero padded (SlabForm::row_pad)
  SlabReduce* reduce = nullptr;
  // optional: called once the step's kernel, totals and reduction are enqueued, BEFORE their read-back, with the result as
  // it stands on the device (slab form; its entry count still on the device: d_nnz) -- what the caller enqueues and adds to
  // the fetch rides on the step's own host round trip (psmatrix.cpp: the NEXT step's exchange layout and plan)
  std::function<void(const DevMat& result, const long long* d_nnz, ScalarFetch& fetch)> before_fetch;
  // optional: the plan of this step, made by the caller from the all-gathered extents and read back together with the
  // exchange layout (slab_plan_panel_async) -- the step then launches without a read-back of its own (and may keep
  // the plan's buffers for its result)
  SlabPlan* plan = nullptr;
  // the product's thin-operand decision (slab_thin_rule on the entry counts summed over the ranks and the global dimension;
  // psmatrix.cpp panel_slab_multiply): the same on every rank, and what one rank decides for the same product
  int thin = 0;
  int64_t nnz_a = 0;   // entries of the whole left operand (bounds the non-zeros of the halo's columns)
  // optional (slab_multiply with a left halo): called with the fetch of the product's entry count before it runs -- what the
  // caller adds comes back on the same host round trip
  std::function<void(ScalarFetch& fetch)> on_fetch;
};
// (could the tile kernel take a plan with these maxima: psmatrix.cpp decides a panel product before its exchange is over)
bool slab_plan_fits_tile(int max_kn, int max_w);
struct SlabPlan;
// true: slab_multiply with a left halo of these columns, this alignment and this plan will NOT decline (the one predicate it uses itself)
bool slab_multiply_takes_panel(const DevMat& A, const DevMat& B, int left_row_pad, int32_t ka, int32_t kb, const SlabPlan* plan);
// the plan of a panel step from the all-gathered packed extents (record stride `pitch`, extents at d_ext_all): flat
// extent arrays of all `dim` columns are left in gfirst / glast, the plan's sizes on the device in plan.blk_toff[blocks]
// and stats24[16..17] (stats24: 24 zeroed words)
void slab_plan_panel_async(const DevMat& X, const int64_t* d_ext_all, int pitch, int32_t dim, int P, SlabPlan& plan,
                           DevBuf<int32_t>& gfirst, DevBuf<int32_t>& glast, unsigned long long* stats24);
// halo != nullptr: X is this rank's column panel; on success the result is left in fuse.result (not installed)
bool slab_step(DevMat& X, SlabFusion& fuse, double threshold, bool dense_rule, const SlabHalo* halo = nullptr);
// halo exchange of a panel in slab form (psmatrix.cpp ps_slab_step_dist): request record (first row, last row, nnz, nnz),
// packed extents (first | last << 32) + prefix of the spans, runs of the local columns [ja, jb) packed back to back, and
// the layout of the columns a rank needs (extents, run addresses in its own buffer or in the receive buffer)
void slab_request_async(const DevMat& X, int64_t* d_out4, const long long* d_nnz = nullptr);   // (d_nnz: the entry count is still on the device)
void slab_extents_async(const DevMat& X, int64_t* d_ext, int64_t* d_pre);
void slab_pack_runs_async(const DevMat& X, const int64_t* d_pre, int32_t ja, int32_t jb, double* dst);
void slab_halo_layout_async(const int64_t* d_ext_all, const int64_t* d_pre_all, int pitch, int32_t dim, int P, int me,
                            int32_t ka, int32_t kb, const int32_t* d_ra, const int64_t* d_zoff, const double* d_recv,
                            const DevMat& X, int32_t* d_first, int32_t* d_last, unsigned long long* d_addr,
                            const int64_t* d_cnt_all = nullptr, int32_t* d_count = nullptr,   // (statistics: entries per column)
                            const int32_t* h_ra = nullptr, const int64_t* h_zoff = nullptr);   // (host copies of d_ra / d_zoff: passed by value up to 16 ranks, the device arrays are then not read)
// request, extents + prefix sums of the spans and (d_cnt64 != nullptr) entry counts of a panel in one pass
void slab_export_async(const DevMat& X, int64_t* d_out4, const long long* d_nnz, int64_t* d_ext, int64_t* d_pre, int64_t* d_cnt64);
void slab_counts_async(const DevMat& X, int64_t* d_cnt64);
// Slab algebra (kernels.hip, last section): the vocabulary of the solver loops on matrices that stay in slab form -- real,
// unlabelled, square, one rank, FMA arithmetic.  Every function returns false and leaves its operands alone when it
// cannot take them (the caller packs and takes the general path).
bool slab_enter(DevMat& M);   // compressed columns -> slab form in place (false: not run-like, stored zeros, complex ...)
bool slab_multiply(const DevMat& A, const DevMat& B, DevMat& C, double alpha, double threshold, bool dense_rule, const SlabHalo* left = nullptr);
// the arithmetic modes the block path computes: the FMA chain (matrix cores) and, on request, unfused (vector units)
inline bool block_arithmetic_ok() { return options().spgemm_fma == 1 || (options().spgemm_fma == 0 && options().block_unfused != 0); }
bool slab_panels_ok();
void slab_allow_panels(bool on);   // a slab session across ranks: the operands of the slab algebra are column panels (rows != columns)
// complex operands in slab form (FMA arithmetic, option complex_tile; a session that allows them): runs of (re, im) pairs in
// slots aligned to 16 rows -- what the complex MFMA tile kernel reads and writes.  Each returns false when it does not take
// its operands (nothing changed): the caller packs and the compressed-column path does the work.
bool sa_operand_c(const DevMat& M);
// sa_operand_c, or the read-only view of a complex matrix with stored zeros (SlabForm::origin, option stored_zero_views): what
// the products, norms and dots read -- a stored zero is a zero of the run
bool sa_readable_c(const DevMat& M);
// (not_run_like: set when it refused because the columns are not run-like; allow_view false: an input with stored zeros is
// refused as without option stored_zero_views, but keeps its chance to become a view later)
bool slab_enter_c(DevMat& M, bool* not_run_like = nullptr, bool allow_view = true);
long long* slab_view_counts();     // [4] views of operands with stored zeros (slots: counters.inc)
long long* ghash_class_counts();   // [4] groups finished by the grouped LDS-hash kernel, by path (slots: counters.inc)
// forgets everything the grouped path keeps between products (the kept column orders, the table class hints, the dimensions
// whose next product goes to the grouped kernel first): which class a product starts in then no longer depends on the products
// before it
void drop_grouped_caches();
bool slab_multiply_c(const DevMat& A, const DevMat& B, DevMat& C, double alpha, double threshold, bool dense_rule, const SlabHalo* left = nullptr);
// true: slab_multiply_c with a left halo of these columns, this alignment and this plan will NOT decline (the one predicate it uses itself)
bool slab_multiply_c_takes_panel(const DevMat& A, const DevMat& B, int left_row_pad, int32_t ka, int32_t kb, const SlabPlan* plan);
bool slab_add_diagonal_c(DevMat& B, double alpha, int32_t col_offset);                      // slab_extra.hip
bool slab_norm_axpby_c(const DevMat& A, const DevMat& B, double alpha, double beta, double* out);   // slab_extra.hip
// slab_extra.hip: Tk = P + a Tkm2 and R <- R + c Tk in one pass, the values of slab_axpby_c(Tkm2, P, a, 1, 0) followed by
// slab_axpby_c(Tk, R, c, 1, 0) bit for bit (Tk may be P); false: what either call would decline, nothing changed
bool slab_recurrence_step_c(const DevMat& P, const DevMat& Tkm2, DevMat& Tk, DevMat& R, double a, double c);
// slab_extra.hip: dot = (Re, Im) of sum conj(A) B for a complex slab-form A and a complex B in slab form or packed compressed
// columns (B == nullptr: none), trace = sum of the real parts of A's diagonal (col_offset: A's first column); fixed-shape sums
bool slab_dot_trace_c(const DevMat& A, const DevMat* B, int32_t col_offset, double dot[2], double* trace);
bool slab_axpby(const DevMat& A, DevMat& B, double alpha, double beta, double threshold);   // B <- alpha A + beta B
bool slab_axpby_to(const DevMat& A, const DevMat& B, DevMat& Out, double alpha, double beta, double threshold);   // Out = alpha A + beta B
bool slab_clone(const DevMat& A, DevMat& Out);
bool slab_scale(DevMat& A, double c);
bool slab_dot(const DevMat& A, const DevMat& B, double out[2]);
bool slab_norm(const DevMat& A, double* out);   // max column abs-sum
// the same on complex matrices in slab form (complex sessions)
bool slab_axpby_c(const DevMat& A, DevMat& B, double alpha, double beta, double threshold);
bool slab_axpby_to_c(const DevMat& A, const DevMat& B, DevMat& Out, double alpha, double beta, double threshold);
bool slab_clone_c(const DevMat& A, DevMat& Out);
bool slab_scale_c(DevMat& A, double c);
bool slab_norm_c(const DevMat& A, double* out);
bool slab_gershgorin(const DevMat& A, int32_t col_offset, double* mn, double* mx);
bool slab_add_diagonal(DevMat& B, double alpha, int32_t col_offset);   // B <- B + alpha I in place (slab_extra.hip); false: not done
// TRS4's polynomial chain on slab-form X and X2 (slab_extra.hip): dot(X2, 4X - 3X2), dot(X2, I - 2X + X2); then the right
// operand (4X - 3X2) + sigma (I - 2X + X2) of the iteration's second product
bool slab_trs4_traces(const DevMat& X, const DevMat& X2, int32_t col_offset, double* trace_fx, double* trace_gx);
bool slab_trs4_operand(const DevMat& X, const DevMat& X2, double sigma, int32_t col_offset, DevMat& Out);
// the same two passes on COMPLEX slab-form X and X2 (k_sa_trs4<double2, .>: every scalar of the chain is real, so each part of an entry goes
// through the real kernel's arithmetic on its own; the traces are Re sum conj(x2) fx and Re sum conj(x2) gx; an entry of the
// operand exists where either part is not zero).  false: not taken (trs4_operands_c) or, for the operand, hulls beyond the
// output's bound -- nothing changed
bool trs4_operands_c(const DevMat& X, const DevMat& X2);
bool slab_trs4_traces_c(const DevMat& X, const DevMat& X2, int32_t col_offset, double* trace_fx, double* trace_gx);
bool slab_trs4_operand_c(const DevMat& X, const DevMat& X2, double sigma, int32_t col_offset, DevMat& Out);
bool slab_norm_axpby(const DevMat& A, const DevMat& B, double alpha, double beta, double* out);   // MatrixNorm(alpha A + beta B), nothing built
// The transpose of a slab form (slab_extra.hip; option slab_transpose).  slab_transpose_operand: what the pass takes -- a square,
// zero-free slab form on one rank that is neither labelled nor a view, packed runs (row_pad 1) or slots aligned to a multiple of
// 16 rows.  slab_transpose<T> (T = double or double2, the operand's kind): AT = A^T, with conj its conjugate, as a fresh slab form
// with A's row_pad whose extents are the first and last non-zero row and whose count is the number of non-zero entries -- packed,
// the pattern and bits of transpose() (then conjugate()) on the packed operand.  false: not taken, or refused because the
// transposed extents need more than 4 A.slots + 4 row_pad n slots; AT is then untouched.  slab_transpose_any picks T.
// slab_conjugate_c: ConjugateMatrix of a zero-free complex slab form in place (false: not taken)
bool slab_transpose_operand(const DevMat& A);
template <typename T>
bool slab_transpose(const DevMat& A, bool conj, DevMat& AT);
bool slab_transpose_any(const DevMat& A, bool conj, DevMat& AT);
bool slab_conjugate_c(DevMat& A);
// Column dot passes for the traces of CGSolver (cg_dots.hip; option cg_dots).  For every local column j and pair (U, V): d_j = the
// chain over ascending row k of conj(U(k, j)) V(k, j) in the product kernels' arithmetic (fma: option spgemm_fma != 0; complex: the
// reference's multiply-add), kept iff |d_j| > threshold (strict, the modulus for complex), else 0 -- entry (j, j) of
// MatrixMultiply(U^H, V, threshold).  out[p] = the sum of the real parts of pair p's d_j in the order of trace() on compressed
// columns: MatrixTrace of that product on this rank, bit for bit.  Rows are global in both operands, so no column offset enters.
// slab_cg_dots: operands in slab form (one pair with U2 == V2 == nullptr); gates: every operand expanded and not labelled, one kind
// and shape (the slots' alignment does not matter: a run is addressed by first / last / off alone); a read-only view is readable
// (its stored zeros are zeros of the run).  false: not taken, out untouched.
// diag != nullptr: the d_j of the FIRST pair copied to that host array (cols doubles).
// cg_dots_columns: the same chains and sums for one pair in packed compressed columns (a merge of the two columns' row lists);
// diag as above.
bool slab_cg_dots(const DevMat& U1, const DevMat& V1, const DevMat* U2, const DevMat* V2, double threshold, double out[2], double* diag = nullptr);
double cg_dots_columns(const DevMat& U, const DevMat& V, double threshold, double* diag = nullptr);
// PowerBounds on one vector (power_vector.hip; option power_vector).  PowerGather: the rows of A (for every row i the pairs
// (k, A(i, k)) in ascending k) in slices of 64 rows, column-major within a slice: entry t of row r lies at soff[r / 64] + 64 t +
// r % 64 of idx / val; a slice is padded to its longest row with (0, 0), which the kernels mask by len[r].
// power_gather_build: from the compressed columns of A (a rank's panel: all rows, its own columns; koff = its first column, added
// to every k), by a stable 32-bit sort of the entries' positions by row -- ascending k within a row, as transpose() orders them;
// false: 32-bit indices do not suffice or the device cannot hold the form -- G is then unusable.
// power_vector_chains: y_i = the chain over ascending k of A(i, k) x(k) in the product kernels' arithmetic (fma: option
// spgemm_fma != 0; complex: the reference's multiply-add); tail: and the product's pruning (|y_i| > threshold, else 0) with the
// workgroups' partial sums in part (3 per block of power_vector_blocks(n)).  power_vector_tail: pruning and partial sums for a y
// that holds unpruned sums (several ranks).  power_vector_finish: out = (sum conj(x) x, Re sum conj(x) y, sum |y|, 1 / that),
// summed in a fixed order.  power_vector_scale: x = y * out[3], pruned slots 0.  Everything on the engine stream, no host wait.
struct PowerGather {
  int32_t n = 0, nslices = 0;
  bool cplx = false;
  int64_t entries = 0;      // padded entries
  DevBuf<int32_t> len;      // 64 nslices: entries of row r (0 beyond n)
  DevBuf<int64_t> soff;     // nslices + 1
  DevBuf<int32_t> idx;
  DevBuf<double> val;
};
bool power_gather_build(const DevMat& A, int32_t koff, PowerGather& G);
int power_vector_blocks(int32_t n);
void power_vector_chains(const PowerGather& G, const double* x, double* y, double threshold, bool fma, bool tail, double* part);
void power_vector_tail(int32_t n, bool cplx, const double* x, double* y, double threshold, double* part);
void power_vector_finish(int32_t n, const double* part, double* out);
void power_vector_scale(int32_t n, bool cplx, const double* y, const double* out, double* x);
// The polynomial chain of the square-root step on slab-form X and X2 = X X (slab_extra.hip k_sa_isr_chain; real or complex, square
// or column panels with col_offset = the panel's first column), the values and patterns of the vocabulary calls at threshold 0 bit
// for bit.  Order 5: Temp2 = (X2 + a X) + (X + b I), Temp = (X2 + a X) + c I (Temp may be X2).  Order 3: Out = 0.375 X2 + (I - X / 2)
// (Out may be X).  false: refused (not in slab form, a view or stored zeros, labelled, different alignments, runs far apart, a
// scaled entry that underflows to zero), nothing changed
bool slab_isr_chain5(const DevMat& X, const DevMat& X2, double a, double b, double c, int32_t col_offset, DevMat& Temp2, DevMat& Temp);
bool slab_isr_chain3(const DevMat& X, const DevMat& X2, int32_t col_offset, DevMat& Out);
// HPCP purification on slab-form matrices (slab_extra.hip; real, square or column panels with col_offset = the panel's first column).
// slab_hpcp_traces: out2 = the LOCAL sums of the diagonals of DDH and D2DH, each with the bits slab_trace gives.  slab_hpcp_update:
// OutD1 = (D1 + 2 D2DH) + (-2 sigma) DDH and OutDH = -(OutD1 + (-1) I) as fresh slab-form matrices, the values and patterns of the
// vocabulary calls at threshold 0 bit for bit, *energy = the LOCAL dot(OutD1, WH) (WH: zero-free slab form or a read-only view).
// false: refused (an operand not in zero-free slab form, labelled, different alignments, runs far apart, a scaled entry that
// underflows to zero), nothing changed
bool slab_hpcp_traces(const DevMat& DDH, const DevMat& D2DH, int32_t col_offset, double out2[2]);
bool slab_hpcp_update(const DevMat& D1, const DevMat& DDH, const DevMat& D2DH, double sigma, const DevMat& WH, int32_t col_offset, DevMat& OutD1,
                      DevMat& OutDH, double* energy);
// the same two passes on COMPLEX slab-form operands (option complex_hpcp; k_hpcp_traces<double2>, k_hpcp_update<double2, .>: runs of
// (re, im) pairs, 16 bytes per lane).  The traces are the sums of the real parts of the diagonals (MatrixTrace); every scalar of
// the update is real, so each merge scales and adds part by part and keeps an entry where either part is not zero -- the values
// and patterns of the vocabulary calls on complex matrices at threshold 0 bit for bit; *energy = Re dot(OutD1, WH), each product
// and each pair's sum rounded (the terms of slab_dot_trace_c, in another fixed order).  The three merged operands: sa_operand_c and
// zero-free; WH: zero-free or a read-only view; slots and the bound count pairs.  false: refused, nothing changed
bool slab_hpcp_traces_c(const DevMat& DDH, const DevMat& D2DH, int32_t col_offset, double out2[2]);
bool slab_hpcp_update_c(const DevMat& D1, const DevMat& DDH, const DevMat& D2DH, double sigma, const DevMat& WH, int32_t col_offset, DevMat& OutD1,
                        DevMat& OutDH, double* energy);
// ScaleAndFold on slab-form matrices (slab_extra.hip; real, square or column panels with col_offset = the panel's first column).
// slab_saf_update: Out = b X + a X2 as a fresh slab-form matrix, the values and pattern of ScaleMatrix(X, b); IncrementMatrix(X2, X, a)
// at threshold 0 bit for bit, *dot = the LOCAL dot(Out, WH) (WH: zero-free slab form or a read-only view; another summation order
// than slab_dot's), *trace = the LOCAL sum of Out's diagonal with the bits slab_trace gives on Out.  slab_saf_dot_trace: the same
// two sums of X as it stands, one pass over X and WH.  One host read-back each.  false: refused (an operand not in zero-free slab
// form, labelled, different alignments, a or b not finite, runs far apart, a scaled entry that underflows to zero), nothing changed
bool slab_saf_update(const DevMat& X, const DevMat& X2, double a, double b, const DevMat& WH, int32_t col_offset, DevMat& Out, double* dot,
                     double* trace);
bool slab_saf_dot_trace(const DevMat& X, const DevMat& WH, int32_t col_offset, double* dot, double* trace);
// the fold update on COMPLEX slab-form operands (option complex_scale_fold; k_saf_update<double2, .>: runs of (re, im) pairs, 16
// bytes per lane).  Both factors are real, so the scaling and the merge work part by part and keep an entry where either part is
// not zero -- the values and pattern of the two vocabulary calls on complex matrices at threshold 0 bit for bit; *dot = Re dot(Out,
// WH), each product and each pair's sum rounded (the terms of slab_dot_trace_c, in another fixed order), *trace = the sum of the
// real parts of Out's diagonal with the bits slab_dot_trace_c gives on Out.  X and X2: sa_operand_c and zero-free; WH: zero-free or
// a read-only view; slots and the bound count pairs.  The scale branch's pass on complex operands is slab_dot_trace_c itself
bool slab_saf_update_c(const DevMat& X, const DevMat& X2, double a, double b, const DevMat& WH, int32_t col_offset, DevMat& Out, double* dot,
                       double* trace);
// The tail of a Heun trial of the WOM solvers on slab-form matrices (wom_heun.hip; real, square or column panels).  slab_wom_heun:
// Out = RK2 = (W + c K0) + c K1 with c = h * 0.5, every merge at `thr` by AddSparseVectors' rules with each link's "other operand's
// last row" the last KEPT row of the link before -- the values and pattern of CopyMatrix(W, RK2); IncrementMatrix(K0, RK2, c, thr);
// IncrementMatrix(K1, RK2, c, thr) bit for bit; *err = the LOCAL MatrixNorm of RK1 - RK2 and *err2 of RK2 - W, both merged at thr,
// with the bits slab_norm gives on those differences in slab form.  One pass over the four runs, one host read-back.  false:
// refused (an operand not in zero-free slab form, labelled, a view, alignments that are no multiples of one another, h or thr not finite, runs far apart, a
// kept value that is exactly zero), nothing changed.  slab_wom_heun_register_rows(): the hull of a column's four runs up to which
// the kernel holds the column in registers; longer columns read their runs once per sweep
bool slab_wom_heun(const DevMat& W, const DevMat& K0, const DevMat& K1, const DevMat& RK1, double h, double thr, DevMat& Out, double* err,
                   double* err2);
int slab_wom_heun_register_rows();
// out[0] = the LOCAL dot(X, W), out[1] = the LOCAL dot(W, XA), each with the bits of slab_dot, from one kernel and one read-back
bool slab_wom_c_dots(const DevMat& X, const DevMat& W, const DevMat& XA, double out[2]);
// The tail of an iteration of PurificationExtrapolate on slab-form matrices (purify_tail.hip; real, square or column panels), D the
// working density, N = D S D the product's output, S the overlap.  fold: Out = N' = 2 D - N as a fresh slab-form matrix, the values
// and pattern of ScaleMatrix(N, -1); IncrementMatrix(D, N, 2) bit for bit; otherwise N' = N and nothing is written.  *norm = the
// LOCAL MatrixNorm of D - N' merged at threshold 0 with the bits slab_norm gives on that difference in slab form; dot = the LOCAL
// DotMatrix(N', S) with the bits of slab_dot(N', S).  One pass over the three runs, one host read-back.  false: refused (D or N not
// in zero-free slab form, labelled, a view, alignments that differ, an S that is neither a zero-free slab form nor a read-only
// view, runs far apart, an input that is not finite, a kept value that is exactly zero), nothing changed
bool slab_purify_tail(const DevMat& D, const DevMat& N, const DevMat& S, bool fold, DevMat& Out, double* norm, double dot[2]);
// The two groups of merges of ComputeExponentialPade on slab-form matrices (pade_chain.hip; real, square or column panels): for
// q = 1, 2  Out_q = CopyMatrix(Base); ScaleMatrix(Out_q, scales[q - 1]); IncrementMatrix(addends[k], Out_q, coeffs[(q - 1) n_addends
// + k], threshold 0) for k = 0 .. n_addends - 1 (n_addends 1 or 3), values and patterns of the calls bit for bit, both outputs as
// fresh slab-form matrices from ONE pass over the inputs' runs and one host read-back.  false: refused (an operand that is not a
// zero-free, unlabelled slab form or is a view, operands named twice, alignments that differ, another n_addends, a scalar that is
// zero or not finite, runs far apart, an input that is not finite, a scaled value that is exactly zero where an entry is held),
// nothing changed
bool slab_pade_chain(const DevMat& Base, const DevMat* const* addends, int n_addends, const double scales[2], const double* coeffs, DevMat& Out1,
                     DevMat& Out2);
// The tail of a step of the Chebyshev / Hermite recurrences on slab-form matrices (poly_step.hip; real, square or column panels):
// Tk = what IncrementMatrix(Q, P, a, threshold 0) leaves in P, Rout = what IncrementMatrix(Tk, R, c, threshold 0) then leaves in R,
// values and patterns of the two calls bit for bit, both as fresh slab-form matrices from ONE pass over the runs of P, Q and R
// (Tk passes from the first merge to the second in a register) and one host read-back.  The outputs' slots are aligned to the
// largest row_pad of the three.  false: refused (an operand that is not a zero-free, unlabelled slab form or is a view, operands
// named twice, a largest alignment that is no multiple of the others, a scalar that is zero or not finite, runs far apart, an
// input that is not finite, a scaled value that is exactly zero where an entry is held), nothing changed
bool slab_poly_step(const DevMat& P, const DevMat& Q, const DevMat& R, double a, double c, DevMat& Tk, DevMat& Rout);
// The scaled sum chain of the solver loops on slab-form matrices (sum_chain.hip; all operands real or all complex -- runs of (re, im)
// pairs, every scalar real and applied to each part by itself, an entry held iff it is not (0, 0) --, square or column panels):
// Out = CopyMatrix(Base); ScaleMatrix(Out, s); IncrementMatrix(addends[k], Out, coeffs[k], threshold 0) for k = 0 .. n_addends - 1
// (n_addends 1 .. 5); ScaleMatrix(Out, post) -- values and pattern of the calls bit for bit (s == 1 and post == 1 stand for no
// scaling call), as ONE fresh slab-form matrix from ONE pass over the inputs' runs and one host read-back.  Out is written only
// on success and may be Base's own DevMat.  false: refused (an operand that is not a zero-free, unlabelled slab form or is a view,
// operands named twice, alignments that differ, another n_addends, a scalar that is zero or not finite, runs far apart, an input
// that is not finite, a scaled value that is exactly zero where an entry is held), nothing changed
bool slab_sum_chain(const DevMat& Base, double s, const DevMat* const* addends, const double* coeffs, int n_addends, double post, DevMat& Out);
// PM purification on a slab-form iterate (slab_extra.hip).  The rows of each column that compressed columns would hold as STORED
// ZEROS (a1 = 0 when sigma > 1/2, unfiltered tails that underflow) travel next to the zero-free runs: rows row[off[j] .. off[j + 1])
// of column j, ascending, disjoint from the run's non-zeros.  off.p == nullptr: no such row.
struct ZeroList {
  DevBuf<int64_t> off;   // cols + 1
  DevBuf<int32_t> row;
  int64_t count = 0;
  void clear() { off.release(); row.release(); count = 0; }
};
// trace and dot(., X) of CopyMatrix(X, Temp); IncrementMatrix(X2, Temp, -1, thr) without forming Temp: LOCAL sums, out2 = (trace, dot)
bool slab_pm_sigma(const DevMat& X, const ZeroList& Z, const DevMat& X2, double thr, int32_t col_offset, double out2[2]);
// ScaleMatrix(X, a1); IncrementMatrix(X2, X, a2, thr); IncrementMatrix(X3, X, a3, thr) in one pass: Out (zero-free runs) and Zout;
// false: refused (operands not in slab form / labelled / a view, or a union extent beyond the output), nothing changed
bool slab_pm_update(const DevMat& X, const ZeroList& Z, const DevMat& X2, const DevMat& X3, double a1, double a2, double a3, double thr,
                    DevMat& Out, ZeroList& Zout);
// the two passes on COMPLEX slab-form operands (option complex_pm; k_pm_sigma<double2>, k_pm_update<double2, ., .>: runs of (re, im)
// pairs, 16 bytes per lane; slots and the bound count pairs).  Every scalar is real, so scalings and sums work part by part; an
// entry is present where either part is not zero or its row is listed, kept where its modulus (Sc<double2>::mag, as the merge on
// compressed columns takes it) exceeds thr or in a tail, and a kept (0, 0) goes to Zout -- the values and pattern of the vocabulary
// calls on complex matrices bit for bit.  out2 = (the real parts of Temp's diagonal summed, Re dot(Temp, X)).  Operands:
// sa_operand_c and zero-free
bool slab_pm_sigma_c(const DevMat& X, const ZeroList& Z, const DevMat& X2, double thr, int32_t col_offset, double out2[2]);
bool slab_pm_update_c(const DevMat& X, const ZeroList& Z, const DevMat& X2, const DevMat& X3, double a1, double a2, double a3, double thr,
                      DevMat& Out, ZeroList& Zout);
// compressed columns with the list's rows inserted as stored zeros (M packed, real or complex); every entry of both is kept
void insert_stored_zeros(DevMat& M, const ZeroList& Z);
// the stored pattern of a packed matrix as a zero list (the diagnostic entry point's Z), and a list as a matrix of stored zeros
// of either kind
void zero_list_from_pattern(const DevMat& M, ZeroList& Z);
DevMat zero_list_matrix(const ZeroList& Z, int32_t rows, int32_t cols, bool cplx = false);
bool slab_trace(const DevMat& A, int32_t col_offset, double* out);   // sum of the diagonal entries held by the local columns
int64_t slab_span_sum(const DevMat& M);   // rows covered by the runs (cached in the form)
long long slab_product_count(const DevMat& A, const DevMat& B);   // statistics (slab_extra.hip): intermediate products of A B
// compressed columns -> labelled slab form (SlabForm::lab; Xs = the matrix in the bandwidth-reducing order, lab[index] = the
// caller's index); false (nothing changed): its columns are not run-like
bool slab_from_csc(DevMat& Xs, DevBuf<int32_t>& lab);
// Operands that arrive relabelled (a band hidden by a symmetric permutation): relabel_enter finds a bandwidth-reducing
// order from the pattern of D (cached per operand, also when nothing was found), renames X into it and turns it into
// labelled slab form; relabelled_operand(D) = D in that order (the cache's copy) or nullptr.  The steps then follow
// the caller's labels (kernels.hip, SlabFuseArgs::lab), pack() renames back.  One rank, real operands.
bool relabel_enter(DevMat& X, const DevMat& D);
const DevMat* relabelled_operand(const DevMat& D);
void relabel_giveup(const DevMat& D);
void drop_thin_transposes();   // (spgemm_thin.hip: the transposes kept per thin left operand)
void drop_operand_caches();   // frees what the fused / relabelled TRS2 paths keep between solves
// band_scope.cpp: while a solve runs on operands redistributed in a recovered band order across ranks, the caller's label of every
// position (device, one per row of the matrices; nullptr outside such a solve).  The fused TRS2 panel steps then decide the
// "beyond the other column's last entry" cases of their merges on these labels, as the one-rank steps on a relabelled operand
// do (SlabForm::lab): the several-rank solve keeps the entries the one-rank solve keeps.
void set_scope_labels(const int32_t* lab);
const int32_t* scope_labels();
void drop_pending_exchange(); // psmatrix.cpp: the exchange layout a panel step prepared for a successor that never came
// relabel.hip: a bandwidth-reducing order of a symmetric pattern (Cuthill-McKee, breadth-first levels on the device):
// newpos[old index] = new index, *bandwidth = max |new row - new column|.  false: not a square packed matrix, or
// more components than the search is willing to chain
bool find_band_order(const DevMat& A, DevBuf<int32_t>& newpos, int64_t* bandwidth);
// sum over the columns of (last row - first row + 1) of a matrix in compressed columns (how run-like it is as it stands)
int64_t column_span_sum(const DevMat& A);
// order-independent fingerprint of a sparsity pattern (compressed columns)
unsigned long long pattern_fingerprint_of(const DevMat& A);
// counters of the multiply paths (slots: counters.inc): fused TRS2 steps, complex TRS2 steps in slab or block form, the two-block
// geometry, the tile-skip test (that one since the last reset_spgemm_accum)
long long* fusion_counts();
long long* complex_fusion_counts();
long long* tile2_counts();
long long* tile_skip_counts();
long long& band_searches();   // searches for a bandwidth-reducing order since start (one per sparsity PATTERN: relabel_enter)

// B <- alpha*A + B (AddSparseVectors semantics), same shape and scalar type.
void increment(const DevMat& A, DevMat& B, double alpha, double threshold);
// the same with the rule applied per block of `row_block` rows (the reference adds distributed matrices block by
// block: whether "the other column is exhausted" is decided inside each row block)
void increment_blocked(const DevMat& A, DevMat& B, double alpha, double threshold, int32_t row_block);
// B <- alpha*A + beta*B (B scaled first, then the same rules); if D and dot_out are given, also
// dot_out = sum conj(B_new) .* D, evaluated in the same pass
void axpby(const DevMat& A, DevMat& B, double alpha, double beta, double threshold, const DevMat* D, double* dot_out,
           double* trace_out = nullptr, int32_t trace_col_offset = 0);  // trace_out: also trace(B_new), same pass
// the same with the first operand taken from a loose product (its exact nnz is learned on the way and returned)
void axpby(const LooseProduct& A, DevMat& B, double alpha, double beta, double threshold, const DevMat* D, double* dot_out,
           double* trace_out, int32_t trace_col_offset, int64_t* a_nnz_out, bool keep_loose = false);
// keep_loose: B (packed or loose on entry) is left LOOSE -- its columns stay in the slots the merge kernels wrote them
// to and the compaction pass does not run.  Loose matrices (DevMat::loose()) are accepted by spgemm (both operands the
// same matrix: the register-slab path reads the slots directly; otherwise packed copies are made), by the second
// operand of axpby(LooseProduct, ...), by the first operand of dot_trace / trace and by clone(); everything else
// needs pack() first and says so loudly.
DevMat packed_copy(const DevMat& M);
void pack(DevMat& M);
// X <- X * X with the result left loose when the register-slab kernel computes it, out = dot(X_new, D), *trace_out =
// trace(X_new): the sigma < 0 step of TRS2 without a compaction pass.  false: operand types this path does not serve
// (nothing done).
bool square_keep_loose(DevMat& X, double threshold, bool dense_rule, const DevMat& D, double out[2], double* trace_out,
                       int32_t col_offset);
// C = A .* B on the intersection of the patterns (conj_a: conjugate A first)
void pairwise(const DevMat& A, const DevMat& B, DevMat& C, bool conj_a);
// out = sum conj(A) .* B  (out[1] = imaginary part, 0 for real)
void dot(const DevMat& A, const DevMat& B, double out[2]);
// the same, plus trace(A) from the same pass (diagonal = row col_offset + j of local column j)
void dot_trace(const DevMat& A, const DevMat& B, double out[2], double* trace_out, int32_t col_offset);
void grand_sum(const DevMat& A, double out[2]);
// sum of the real parts of entries with row == col + col_offset
double trace(const DevMat& A, int32_t col_offset);
// per-column sum |v| -> out[cols]
void column_abs_sums(const DevMat& A, DevBuf<double>& out);
double max_of(const DevBuf<double>& v, size_t n);
// per-column Gershgorin discs -> min over columns of (d - r), max of (d + r)
void gershgorin(const DevMat& A, int32_t col_offset, double* mn, double* mx);
void scale(DevMat& A, double c);
void conjugate(DevMat& A);
// values of column j *= factor[j] (cols scalars of the matrix' scalar type in device memory)
void scale_columns(DevMat& A, const double* d_factor);
DevMat to_complex(const DevMat& A);
DevMat to_real(const DevMat& A);
// identity restricted to local columns [col_offset, col_offset+cols) of an n x n matrix
DevMat identity(int32_t n, int32_t col_offset, int32_t cols, bool cplx);
// is it exactly the (local part of the) identity?  returns number of diagonal ones or -1
int64_t identity_check(const DevMat& A, int32_t col_offset);
DevMat transpose(const DevMat& A);
// general re-indexing: entry (i, j) -> (row_map[i], col_map[j]) (0-based device maps, may be null
// = identity); entries whose mapped column falls outside [col_lo, col_hi) are dropped, columns are
// stored relative to col_lo; the result is sorted.  drop_exact_zeros mimics a threshold-0 multiply
// with a permutation matrix (LoadBalancerModule.F90:38-47), which prunes stored zeros.
DevMat remap_general(const DevMat& A, const int32_t* d_row_map, const int32_t* d_col_map, int32_t new_rows,
                     int32_t col_lo, int32_t col_hi, bool drop_exact_zeros);
// columns [col_lo, col_hi) of A^T
DevMat transpose_slice(const DevMat& A, int32_t col_lo, int32_t col_hi);
// columns [c0, c1) of A as a new matrix
DevMat column_slice(const DevMat& A, int32_t c0, int32_t c1);
// A with only the columns of one K slice kept (the others empty): column j (global index col_offset + j) is kept when
// ((col_offset + j) / block) % slices == slice -- the share of the inner dimension one process slice of the reference
// multiplies (MatrixMultiply.f90:74-80, 102-110)
DevMat mask_columns(const DevMat& A, int32_t col_offset, int32_t block, int32_t slices, int32_t slice);
// concatenate column panels (all with the same rows / scalar type)
DevMat concat_columns(const std::vector<const DevMat*>& parts);

DevMat from_triplets(const HostTriplets& t, int32_t rows, int32_t cols, int32_t col_offset);
void to_triplets(const DevMat& A, int32_t col_offset, HostTriplets& out);

// dst[i] = src[i] + shift for i < count
void copy_shift_i64(const int64_t* d_src, int64_t* d_dst, int64_t count, int64_t shift);

// dst[i] = src[i] - src[0] + add ; dst[i] = v ; first/last stored row over all columns (INT_MAX / -1 if empty)
void rebase_i64(const int64_t* d_src, int64_t* d_dst, int64_t count, int64_t add);
void fill_i64(int64_t* d_dst, int64_t count, int64_t v);
void row_range(const DevMat& A, int32_t* lo, int32_t* hi);
// device-side pieces of the halo-exchange plan (comm.cpp gather_needed): no host round trip of their own
void halo_request_async(const DevMat& B, int64_t nnz_a, int64_t* d_out4);
// interior columns of a B panel (empty, or every row in [c0, c1)): d_out5 = {first interior column, last interior
// column, number of interior columns, entry offset of the first, entry offset one past the last}
void halo_interior_async(const DevMat& B, int32_t c0, int32_t c1, int64_t* d_out5);
// the P x P count matrix and my send bounds from the gathered requests and the gathered panel offsets (one kernel)
void halo_counts_async(const int64_t* d_req, const int64_t* d_outer_all, int pitch, int32_t dim, int P, int me, int64_t* d_cnt,
                       int64_t* d_bound);
void halo_bounds_async(const DevMat& A, int32_t c0, const int32_t* d_sa, const int32_t* d_sb, int P, int64_t* d_bound,
                       int64_t* d_cnt_row);

// C = alpha A B for a thin left operand (spgemm_thin.hip); false: not taken (C untouched).  dense_rule_bits: bit 0 the
// dense branch's order of threshold and alpha, bit 1 fma accumulation (real operands)
bool spgemm_thin_left(const DevMat& A, const DevMat& B, DevMat& C, double alpha, double threshold, int dense_rule_bits, int64_t* products,
                      hipEvent_t ev_begin, hipEvent_t ev_end);
// thin operands inside a slab session (spgemm_thin.hip; FMA arithmetic, real or complex): the plan's block windows and output
// slots, B (and, thin right operand, A) as the runs of the slab form, a thin left operand as the compressed columns of its
// transpose.  Complex: the value pointers name (re, im) pairs, offsets and slots count elements.
struct ThinSlabArgs {
  const int32_t *blk_lo = nullptr, *blk_w = nullptr;
  const int64_t* blk_toff = nullptr;
  const int32_t *bfirst = nullptr, *blast = nullptr;
  const int64_t* boff = nullptr;
  const double* bval = nullptr;
  const int32_t *afirst = nullptr, *alast = nullptr;
  const int64_t* aoff = nullptr;
  const double* aval = nullptr;
  const int64_t* at_outer = nullptr;
  const int32_t* at_inner = nullptr;
  const double* at_val = nullptr;
  double* out_val = nullptr;
  int32_t *count = nullptr, *ofirst = nullptr, *olast = nullptr;
  int64_t* ooff = nullptr;
  double alpha = 1.0, threshold = 0.0;
  int dense_rule = 0, ncols = 0, nrows = 0;
  int* flag = nullptr;   // thin right operand, real: raised when a column lists more non-zeros than the kernel holds
  // a panel product (thin right operand): afirst / alast / aaddr are indexed by GLOBAL column numbers (biased pointers),
  // aaddr[k] = address of the first row of the run of A's column k (SlabHalo::addr); aoff / aval are then unused
  const unsigned long long* aaddr = nullptr;
  int nblocks = 0;       // > 0: ooff[ncols] = blk_toff[nblocks] is written too (the complex slab form, as its tile kernel does)
};
void launch_thin_slab(const ThinSlabArgs& a, bool left, bool cplx = false);
// the rows of a thin left operand given as the runs of its columns ka .. kb - 1 (first / last / addr or off indexed by global
// column number; addr == nullptr: run k starts at base + off[k] elements) as compressed columns of its transpose, entries in
// ascending k; cap: an upper bound of the non-zeros (the operand's entry count).  Asynchronous, no host round trip.
struct ThinRows {
  DevBuf<int64_t> outer;
  DevBuf<int32_t> inner;
  DevBuf<double> val;
};
void thin_rows_from_runs(bool cplx, const int32_t* first, const int32_t* last, const unsigned long long* addr, const int64_t* off,
                         const double* base, int32_t ka, int32_t kb, int32_t nrows, int64_t cap, ThinRows& out);
// which gather kernel a product of a slab session takes (0: none, 1: thin left operand, 2: thin right operand) -- from the
// GLOBAL entry counts and the global dimension, so that every rank of a panel product, and one rank alone, decide alike
inline int slab_thin_rule(int64_t nnz_a, int64_t nnz_b, int64_t dim) {
  return (nnz_a <= 8 * dim && nnz_b >= nnz_a) ? 1 : (nnz_b <= 8 * dim) ? 2 : 0;
}
long long* thin_slab_counts();   // [6] products of slab sessions on the gather kernels (slots: counters.inc)
// counts the operations that change the values of a matrix in place (scale, conjugate, ...): together with the serial
// number of the value buffer's allocation it tells whether a cached derivative of a matrix is still that matrix
unsigned long long matrix_value_epoch();
void bump_matrix_value_epoch();
// compressed columns without the merge pass (column_fused.hip): B <- B + alpha I in place when every local column stores its
// diagonal entry (global columns c0 ...); max column abs-sum of alpha A + B without forming it.  false: not taken
bool add_identity_inplace(DevMat& B, double alpha, int32_t c0);
bool norm_axpy_columns(const DevMat& A, const DevMat& B, double alpha, double* norm);
// exclusive scan helper (device), out[n] = total; returns total (synchronises)
// dense side (dense.hip): entry filter, sparse <-> dense (column major), Hermitian eigendecomposition (parallel
// two-sided Jacobi), (pivoted) Cholesky on a dense copy
DevMat filter(const DevMat& A, double threshold);  // entries with |v| > threshold
void to_dense(const DevMat& A, double* d_dense, int64_t ld);
DevMat from_dense(const double* d_dense, int64_t ld, int32_t rows, int32_t c0, int32_t cols, bool cplx, double threshold);
void dense_zero_columns(double* d_dense, int64_t ld, int32_t rows, int32_t c_first, int32_t c_end, bool cplx);
void dense_eigh(double* d_A, int32_t n, bool cplx, double* d_W);
void dense_cholesky(const double* d_A, double* d_L, int32_t n, double threshold, int32_t rank);
int64_t exclusive_scan_i64(const int64_t* d_in, int64_t* d_out, int64_t n);
// the same without the read-back: out[0..n] = exclusive prefix sums, out[n] = total; asynchronous on the engine stream
void scan_i32_async(const int32_t* d_in, int64_t* d_out, int64_t n);
void scan_i64_async(const int64_t* d_in, int64_t* d_out, int64_t n);
// the reductions behind slab_dot and slab_norm for passes in other translation units, asynchronous on the engine stream: out2[0]
// = the deterministic two-level sum of the first members of n (x, y) pairs, out2[1] = of the second; out2[1] = the maximum of v[0..n)
void reduce_sum_pairs_async(const double* part, int n, double* out2);
void reduce_max_async(const double* v, int64_t n, double* out2);

}  // namespace ntp
