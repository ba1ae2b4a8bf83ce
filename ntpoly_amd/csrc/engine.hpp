// Host-side engine: process grid, distributed matrix (column panels, one per GPU),
// distributed algebra, solver parameters, convergence monitor, logger and the solvers.
// Mirrors the reference's module API (names cite the Fortran modules) in C++ because the
// reference host is compiled code; the C ABI in wrp.cpp is the reference's own *_wrp surface.
#pragma once
#include <cstdio>
#include <string>
#include <functional>
#include <initializer_list>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace ntp {

// ------------------------------------------------------------------ communication
// One communicator over all ranks (one process per GPU).  nranks == 1 needs no transport.
// The data plane is RCCL over xGMI.  A second transport exists for TESTS only (NTPOLY_AMD_COMM=shm:<name>): the
// ranks are processes sharing ONE GPU and exchange through a POSIX shared-memory segment, which lets the multi-rank
// code paths (halo exchange, panel gathers, distributed solvers) run on a single-GPU box.
struct Transport {
  virtual ~Transport() {}
  // all pointers are device pointers; sizes in bytes; operations are ordered on the engine stream
  virtual void allgather(const void* send, void* recv, size_t bytes_per_rank) = 0;
  virtual void allreduce(void* buf, size_t count, bool is_f64, int op /*0 sum, 1 min, 2 max*/) = 0;
  virtual void bcast(const void* send, void* recv, size_t bytes, int root) = 0;
  virtual void group_begin() = 0;
  virtual void send(const void* p, size_t bytes, int peer) = 0;
  virtual void recv(void* p, size_t bytes, int peer) = 0;
  virtual void group_end() = 0;
  // stream the following point-to-point group is enqueued on (RCCL); the shared-memory test transport is synchronous
  virtual void set_stream(hipStream_t) {}
  // a transport over the sub-group `members` (ranks of THIS transport, ascending new rank; this rank is members[new_rank]);
  // collective over this transport's ranks: every rank calls it with its own colour (RCCL: ncclCommSplit)
  virtual Transport* split(int color, int key, int new_rank, const std::vector<int>& members) = 0;
};
struct Comm {
  int rank = 0, nranks = 1;
  Transport* tr = nullptr;
  bool force = false;    // tests: run the multi-rank code paths even with a single rank
  bool user_init = false;  // ntpoly_amd_init_comm was called (also with one rank): the caller's MPI communicator is not consulted
  bool retired = false;    // a sub-communicator whose transport comm_finalize tore down (the object itself stays)
  bool active() const { return tr != nullptr && (nranks > 1 || force); }
};
// The communicator the engine's collectives run on: the one of the innermost open CommScope, or the one over all processes
// when no scope is open.  Every ps_* and solver entry opens a scope on the grid of the matrix it works on, so on a SUB-grid
// (SplitProcessGrid / CommSplitMatrix, ProcessGridModule.F90:430-515) the multiply, the reductions and the solvers stay inside
// that half, and nothing a call selected outlives it.
Comm& world();
Comm& base_world();                 // the communicator over all processes, whatever is selected
// MPI_Comm_split on the current communicator (collective): the ranks of one colour, ordered by (key, rank); the result is
// owned by the engine (retired, never freed, by comm_finalize)
Comm* comm_split(int color, int key);
// halo exchanges of the distributed multiply since the start, and the host synchronisations they needed
struct ExchangeStats { long long exchanges = 0, host_syncs = 0; };
ExchangeStats& exchange_stats();
void comm_get_unique_id(char out[128]);
void comm_init(const char id[128], int rank, int nranks);
void comm_finalize();
// ranks from the caller's MPI communicator (Fortran handle), when the process has initialised an MPI library and the
// engine has no communicator yet; true when a multi-rank communicator exists afterwards
bool comm_bind_mpi(int fortran_comm);
void comm_allreduce_sum(double* host_vals, int n);
void comm_allreduce_min(double* host_vals, int n);
void comm_allreduce_max(double* host_vals, int n);
void comm_allreduce_sum_i64(int64_t* host_vals, int n);
void comm_bcast_i32(int32_t* host_vals, int n, int root);
void comm_allgather_i64(const int64_t* mine, int n, int64_t* all /* n * nranks */);
void comm_barrier();

// ProcessGrid_t (ProcessGridModule.F90:15-56).  The reference's rows x columns x slices shape is
// kept for the API (getters, consistency check); the data decomposition of this engine is always
// 1-D column panels over the global rank (DESIGN.md "Multi-GPU").
struct ProcessGrid {
  int num_rows = 1, num_cols = 1, num_slices = 1;
  int my_row = 0, my_col = 0, my_slice = 0;
  int global_rank = 0, total = 1;
  Comm* comm = nullptr;   // the communicator the grid lives on (nullptr: all processes); set by construct_grid
  bool is_root() const { return global_rank == 0; }
};
// Selects the communicator of g (all processes for a null grid or a grid on all of them) until the end of the enclosing
// block, then the one selected before.  A grid whose communicator comm_finalize retired is fatal.
struct CommScope {
  explicit CommScope(const ProcessGrid* g);
  ~CommScope();
  CommScope(const CommScope&) = delete;
  CommScope& operator=(const CommScope&) = delete;
  Comm* prev;
};
// SplitProcessGrid (ProcessGridModule.F90:430-515): two grids of about half the size, preferably along the slices, else along
// the longer of rows / columns; collective over the old grid.  The new grid (owned by the engine) lives on a sub-communicator
// made of the processes of this process's colour in the order of their old ranks.
ProcessGrid* split_process_grid(const ProcessGrid& old_grid, int* my_color, bool* split_slice);
// CommSplitMatrix (PSMatrixModule.F90:1489-1541, distributed_includes/CommSplitMatrix.f90): a copy of the WHOLE matrix on each
// of the two halves of its grid (column panels over the half's processes)
struct PSMatrix;
void ps_comm_split(const PSMatrix& m, PSMatrix& split, int* my_color, bool* split_slice);
ProcessGrid& global_grid();
bool global_grid_constructed();
// a grid over the ranks of c (base_world(): all processes)
void construct_grid(ProcessGrid& g, int rows, int cols, int slices, Comm& c);
void construct_grid_default(ProcessGrid& g, int slices /* <=0: choose */, Comm& c);
void write_grid_info(const ProcessGrid& g);

// ------------------------------------------------------------------ distributed matrix
// Matrix_ps (PSMatrixModule.F90:33-51): rank r owns the column panel [c0, c1) (all rows).
struct PSMatrix {
  const ProcessGrid* grid = nullptr;
  int32_t dim = 0;  // actual == logical dimension (no padding needed for 1-D panels)
  bool cplx = false;
  int32_t c0 = 0, c1 = 0;
  DevMat loc;       // dim x (c1-c0)
  bool constructed() const { return grid != nullptr; }
};
void panel_range(int32_t dim, int nranks, int rank, int32_t* c0, int32_t* c1);
void ps_construct_empty(PSMatrix& m, int32_t dim, const ProcessGrid* g, bool cplx);
void ps_construct_like(PSMatrix& m, const PSMatrix& ref);
void ps_copy(const PSMatrix& a, PSMatrix& b);
// Slab session (psmatrix.cpp): while one is open -- a solver loop, one rank, real operands, FMA arithmetic, option
// slab_algebra -- ps_multiply / ps_axpby / ps_increment / ps_copy / ps_scale / ps_dot / ps_norm / ps_gershgorin keep
// their operands and results in slab form (kernels.hpp, slab algebra) instead of compressed columns; the loop's owner
// packs what leaves it (ps_slab_leave).  Any operation that cannot be done in slab form packs its operands and takes
// the general path; after a handful of refusals the session stays off.
struct SlabSession {
  // api: a one-call session of the C ABI's vocabulary entry points.  complex_ok: the loop's products, identity increments and
  // norms of differences take COMPLEX operands in slab form too (FMA arithmetic, options complex_tile / complex_sessions);
  // every other operation packs them first
  explicit SlabSession(bool eligible, bool api = false, bool complex_ok = false);
  ~SlabSession();
  SlabSession(const SlabSession&) = delete;
  SlabSession& operator=(const SlabSession&) = delete;
  void close();   // (the loop is over: what follows works on compressed columns again)
  bool opened = false;
  bool set_complex = false;
};
// Unfused arithmetic, real operands, until the outermost open session closes: the session's products stay on the register-slab
// kernel also when an operand has become sparse inside wide extents (3 I - a^2 U^T U near the end of a Polar solve), where
// ps_multiply otherwise hands the product to the general kernels and books a refusal that packs both operands.  For the loop that
// transposes its iterate every iteration: a packed iterate sends the next transpose through the sort on compressed columns and the
// next product through the expansion of both operands again.  The kernel multiplies the zeros of the runs, which changes no bit.
// No session open: nothing happens
void slab_keep_sparse_runs(bool on);
// Out = alpha A + beta B: CopyMatrix(B, Out); ScaleMatrix(Out, beta); IncrementMatrix(A, Out, alpha, threshold) -- in a
// slab session one pass without the copy (and B, an identity say, is turned into slab form once instead of its copies)
void ps_copy_axpby(const PSMatrix& B, const PSMatrix& A, PSMatrix& Out, double alpha, double beta, double threshold);
// IncrementMatrix(Identity, B, alpha, 0) where the caller KNOWS its first operand is the identity (built by
// FillMatrixIdentity, possibly under the load balancer's permutation, which leaves it the identity): in a slab session one
// value per column changes in place; otherwise the ordinary merge
void ps_increment_identity(const PSMatrix& Identity, PSMatrix& B, double alpha);
// TRS4's polynomial chain without its intermediates, for an X and X2 in slab form inside a slab session (false: not
// done, the caller runs the sequence of merges and dots): the two traces, then P = Fx + sigma Gx
bool ps_trs4_traces(const PSMatrix& X, const PSMatrix& X2, double* trace_fx, double* trace_gx);
bool ps_trs4_operand(const PSMatrix& X, const PSMatrix& X2, double sigma, PSMatrix& P);
// Option complex_trs4 (one rank, inside a session that takes complex operands): the two calls above take a complex X and X2 in
// complex slab form (slab_extra.hip k_sa_trs4<double2, .>: the real kernel's arithmetic on each part of an entry, the values and pattern of
// the four merges at threshold 0; the traces summed in another fixed order), and
// ps_trs4_energy: *energy = the real part of dot(X, WH) from one pass over the runs of a complex slab-form X and WH as it stands --
// slab form, a read-only view or compressed columns, stored zeros included (slab_dot_trace_c) -- instead of a dot that packs X.
// false: not done, nothing changed -- the caller runs the vocabulary calls.  Gates (the option off, several ranks, no complex
// session, block form, a labelled slab form, an operand still in compressed columns, sigma == 0 for the operand) count nothing;
// past them a pass the kernel does not take (alignments that differ, hulls beyond the output's bound) counts as refused.
// slab_algebra_counts() counts a fused pass as the real branch does.
bool ps_trs4_energy(const PSMatrix& X, const PSMatrix& WH, double* energy);
// DIAGNOSTICS (the C ABI's ntpoly_amd_trs4_chain_step / _trs4_energy): X and X2 (X) are brought into slab form where they are; both
// traces and P, packed, from caller-held matrices -- real ones in any session, complex ones under the gates above; false: gated
// or refused, every matrix as it was
bool ps_trs4_chain_step(const PSMatrix& X, const PSMatrix& X2, double sigma, PSMatrix& P, double* trace_fx, double* trace_gx);
bool ps_trs4_energy_step(const PSMatrix& X, const PSMatrix& WH, double* energy);
long long* complex_trs4_counts();   // (slots: counters.inc)
// PM purification with the iterate X kept in slab form (zero-free runs) and the rows compressed columns would hold as stored
// zeros in Z (kernels.hpp ZeroList; option pm_session), inside a real slab session, one rank or column panels across ranks.
// ps_pm_sigma: trace and dot(., X) of X - X2 merged at `threshold`, X - X2 not formed.  Collective: the two sums and "some rank
// cannot" travel in one reduction; false on EVERY rank then, nothing changed.
// ps_pm_update: X <- a1 X + a2 X2 + a3 X3 as ScaleMatrix and two IncrementMatrix calls, Z <- the new list.  Local: false when THIS
// rank cannot -- it has then materialised its iterate and made the two merges on compressed columns (Z is empty); the caller
// hands that to ps_pm_energy, whose reduction tells every rank.
// ps_pm_energy: dot(X, WH) as ps_dot, with "this rank left the fused path" carried by the same reduction; *some_refused: on any rank.
// ps_pm_materialise: X to compressed columns with Z's rows inserted as stored zeros -- what the loop on compressed columns holds.
// Option complex_pm (one rank, inside a session that takes complex operands): the four calls take COMPLEX operands (slab_extra.hip
// k_pm_sigma<double2>, k_pm_update<double2, ., .>: the real kernels' rules on each part of an entry, the threshold on the modulus as the
// merge on compressed columns takes it -- the values, pattern and stored zeros of the vocabulary calls bit for bit; *trace_value =
// the real parts of the diagonal summed, *dot_value = Re dot(X - X2, X); ps_pm_energy = Re dot(X, WH) from one pass over X's runs
// and WH as it stands: slab_dot_trace_c).  No collective.  *gated (optional): ps_pm_sigma returned false at a gate -- the option
// off, several ranks, no complex session, block or loose form, a labelled slab form, operands that are not all complex and of one
// dimension --, which counts nothing; past the gates an operand that is no zero-free complex slab form (a read-only view, compressed
// columns) or runs far apart refuse.  complex_pm_counts() keeps these books; pm_session_counts() never counts a complex pass,
// slab_algebra_counts() counts a fused pass as the real branch does.
bool ps_pm_sigma(const PSMatrix& X, const ZeroList& Z, const PSMatrix& X2, double threshold, double* trace_value, double* dot_value,
                 bool* gated = nullptr);
bool ps_pm_update(PSMatrix& X, ZeroList& Z, const PSMatrix& X2, const PSMatrix& X3, double a1, double a2, double a3, double threshold);
double ps_pm_energy(const PSMatrix& X, const PSMatrix& WH, bool refused_here, bool* some_refused);
void ps_pm_materialise(PSMatrix& X, ZeroList& Z);
long long* complex_pm_counts();   // (slots: counters.inc)
long long* pm_session_counts();   // (slots [0..3]: counters.inc; [4] the longest zero list an update left on this rank)
// MatrixNorm of alpha A + beta B (ScaleMatrix(B, beta); IncrementMatrix(A, B, alpha, 0); MatrixNorm(B)) for the loops
// that build the sum only for its norm; false: not done (outside a slab session, operands in compressed columns ...)
bool ps_norm_axpby(const PSMatrix& A, const PSMatrix& B, double alpha, double beta, double* norm);
// The recurrence step of the Chebyshev / Hermite loops on complex operands in a complex slab session (option
// complex_poly_sessions = 2): IncrementMatrix(Tkm2, P, a, 0) with its result in Tk (which may be P), then
// IncrementMatrix(Tk, R, c, 0), in one pass (slab_extra.hip slab_recurrence_step_c: the same values bit for bit); false:
// not done and nothing changed -- the caller makes the two ps_increment calls
bool ps_recurrence_step(const PSMatrix& P, const PSMatrix& Tkm2, PSMatrix& Tk, PSMatrix& R, double a, double c);
// The same step on REAL operands inside a real slab session, option poly_step = 2 (poly_step.hip k_poly_step): what
// IncrementMatrix(Tkm2, P, a, 0) leaves in P goes to Tk (which may be P), what IncrementMatrix(Tk, R, c, 0) then leaves in R
// replaces R -- one pass over the runs of P, Tkm2 and R with two fresh outputs and one read-back, values and patterns of the two
// calls bit for bit.  An operand still in compressed columns (the identity as T0, the input as T1, the sum before the first
// product) is turned into slab form where it is.  Counted in slab_algebra_counts() as the two merges replaced.  Local: no
// reduction is entered, and the calls it replaces are local too, so across ranks each panel decides for itself.  false: nothing
// done -- kept out by a gate (the option below 2, no open real session or one that has given up, a complex operand, block form, a
// labelled slab form, dimensions that differ, one matrix in two roles, a == 0 or c == 0, a grid with process slices: counted
// nowhere) or refused (counted in poly_step_counts(): an operand the slab form cannot hold or a view, alignments without a common
// multiple among them, runs far apart, an input that is not finite, a scaled value that is exactly zero where an entry is held)
// -- the caller makes the two ps_increment calls.  ps_recurrence_step is the complex loops' and stays as it is.
bool ps_poly_step(const PSMatrix& P, const PSMatrix& Tkm2, PSMatrix& Tk, PSMatrix& R, double a, double c);
// DIAGNOSTIC (the C ABI's ntpoly_amd_poly_step): the same pass on caller-held matrices with both outputs packed into TkOut and
// ROut, which are none of the inputs and not one another; the inputs keep their values.  One rank only (several ranks are a gate)
bool ps_poly_step_diag(const PSMatrix& P, const PSMatrix& Tkm2, const PSMatrix& R, double a, double c, PSMatrix& TkOut, PSMatrix& ROut);
long long* poly_step_counts();   // (slots: counters.inc)
// The scaled sum chain of the real solver loops inside a real slab session, option sum_chain = 1 (sum_chain.hip k_sum_chain):
//   CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(*addends[k], Out, coeffs[k], 0) for k = 0 .. n_addends - 1;
//   ScaleMatrix(Out, post)
// in one pass over the runs of Base and the addends and one read-back, values and pattern of the calls bit for bit; s == 1 and
// post == 1 stand for no scaling call.  n_addends is 1 .. 5.  Out may be Base (the in-place sequences: the fresh result is
// installed over it) or none of the inputs, never an addend.  The inputs are only read (one still in compressed columns is turned
// into slab form where it is).  Counted in slab_algebra_counts() as the calls replaced.  Local: no reduction is entered, and the
// calls it replaces are local too, so across ranks each panel decides for itself.  false: nothing done -- kept out by a gate (the
// option at 0, no open real session or one that has given up, a complex operand, block form, a labelled slab form, dimensions
// that differ, one matrix in two input roles, Out an addend, n_addends outside 1 .. 5, a grid with process slices, s, post or a
// coefficient that is zero or not finite: counted nowhere) or refused (counted in sum_chain_counts(): an operand the slab form
// cannot hold or a view, alignments that differ, runs far apart, an input that is not finite, a scaled value that is exactly zero
// where an entry is held) -- the caller makes the calls.
bool ps_sum_chain(const PSMatrix& Base, double s, const PSMatrix* const* addends, const double* coeffs, int n_addends, double post, PSMatrix& Out);
// DIAGNOSTIC (the C ABI's ntpoly_amd_sum_chain): the same pass with the result packed.  One rank only (several ranks are a gate)
bool ps_sum_chain_step(const PSMatrix& Base, double s, const PSMatrix* const* addends, const double* coeffs, int n_addends, double post, PSMatrix& Out);
long long* sum_chain_counts();   // (slots: counters.inc)
// The complex side, option complex_sum_chain (independent of sum_chain, as complex_hpcp is of hpcp_step).  1: the inverse-root
// iteration opens a complex slab session as the Taylor square-root loop does ([0] of complex_sum_chain_counts() counts those loops).
// 2: and ps_sum_chain / ps_sum_chain_step also take a chain whose operands are ALL complex, inside an open session that takes complex
// operands (FMA arithmetic, complex_tile, complex_sessions; one rank, or complex column panels): k_sum_chain<double2, M> on runs of
// (re, im) pairs -- every scalar real and applied to each part by itself, the merge part by part, an entry held iff it is not (0, 0),
// the values and the pattern of the vocabulary calls at threshold 0.  Operands enter without views (a stored (0, 0) refuses).  The
// gates are the real branch's, with "the option below 2", "no open session that takes complex operands" and "real and complex
// operands mixed" among them; taken passes count in slab_algebra_counts() as the real branch's, passes and refusals in
// complex_sum_chain_counts() [1] and [2] only -- sum_chain_counts() never moves for complex operands.
long long* complex_sum_chain_counts();   // (slots: counters.inc)
// The polynomial chain of the Taylor square-root step (SquareRootSolversModule.F90:425-479) in one pass over the runs of X and
// X2 = X X (option isr_chain; slab_extra.hip k_sa_isr_chain), inside an open slab session that takes the operands' kind, both in
// slab form.  ps_isr_chain5: what ps_increment(X, T, a, 0); ps_copy_axpby(I, X, Temp2, 1, b, 0); ps_increment(T, Temp2, 1, 0);
// ps_increment_identity(I, T, c) leave in Temp2 and T, with T = X2 on entry and Temp on return (Temp may be X2).
// ps_isr_chain3: what ps_axpby(I, X, 1, -1/2, 0); ps_increment(X2, X, 0.375, 0) leave in X.  The same bits and patterns.  false:
// not done and nothing changed -- the caller makes the calls.  Local to a rank (no collective), and silent: a refusal is not
// a refusal of the session.  Counted in slab_algebra_counts() as the merges replaced (four, two).  Gates (the option off, no open
// session for the operands' kind, X and X2 both in compressed columns, a labelled slab form) return false before anything is
// counted: such a step is neither fused nor refused in isr_chain_counts().  "Nothing changed" holds for values, not for the
// representation: an operand still in compressed columns is turned into slab form where it is before the kernel decides, and stays
// so -- if X enters and X2 cannot (not run-like), the vocabulary calls that follow repeat the failing conversion, count a session
// refusal and pack both: the same bits, at the cost of one conversion more on that path.
bool ps_isr_chain5(const PSMatrix& X, const PSMatrix& X2, double a, double b, double c, PSMatrix& Temp2, PSMatrix& Temp);
bool ps_isr_chain3(PSMatrix& X, const PSMatrix& X2);
// DIAGNOSTIC (the C ABI's ntpoly_amd_isr_chain_step): X and X2 are brought into slab form where they are, one chain of the given
// order runs, the outputs are packed into Out1 (order 5: Temp2, order 3: the new X) and Out2 (order 5: Temp; order 3: untouched)
bool ps_isr_chain_step(const PSMatrix& X, const PSMatrix& X2, int order, double a, double b, double c, PSMatrix& Out1, PSMatrix& Out2);
long long* isr_chain_counts();   // (slots: counters.inc)
// HPCP purification (DensityMatrixSolversModule.F90:839-878) inside a real slab session, option hpcp_step (slab_extra.hip
// k_hpcp_traces / k_hpcp_update).
// ps_hpcp_traces: out = trace(DDH), trace(D2DH), each with the bits of ps_trace, from one pass and one read-back.  Collective: one
// reduction carries both sums; a rank whose panels the kernel does not take adds the partial sums it computes as ps_trace would
// (not counted as fused).  false -- before any collective, by gates that are the same on every rank (the option off, no open real
// session, a complex operand, block form) --: the caller makes the two ps_trace calls.
// ps_hpcp_update: what ps_increment(D2DH, D1, 2, 0); ps_increment(DDH, D1, -2 sigma, 0) leave in D1, *energy = dot(D1, WH), and in
// DH what ps_copy(D1, DH); ps_increment_identity(I, DH, -1); ps_scale(DH, -1) would build from that D1: values and patterns bit
// for bit, the energy to rounding (another summation order; it only feeds the convergence monitor).  Counted in
// slab_algebra_counts() as the four merges / copies and two other operations replaced.  false: not done, D1 and DH as they were
// (an operand still in compressed columns may have been turned into slab form, as in ps_isr_chain5) -- the caller makes the two
// merges and the dot, and builds the next DH with the three calls.  The merges are local to a rank; the energy's reduction has
// the shape of ps_dot's, so a rank that returns false and calls ps_dot meets the other ranks' reduction with its own partial sum:
// every rank enters the same collectives in the same order whichever ranks refuse.  Gates (the option off, no open real session,
// a complex operand, block form, a labelled slab form, all three operands in compressed columns, alignments that differ, a WH
// that is neither a zero-free slab form nor a read-only view) count nothing; a sigma that is zero or not finite (before launch),
// an operand the slab form cannot hold, runs far apart and a scaled entry that underflows to zero count as refused.
bool ps_hpcp_traces(const PSMatrix& DDH, const PSMatrix& D2DH, double out[2]);
bool ps_hpcp_update(PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, double sigma, const PSMatrix& WH, PSMatrix& DH, double* energy);
// DIAGNOSTIC (the C ABI's ntpoly_amd_hpcp_update_step): the operands are brought into slab form where they are, one update runs,
// the new D1 and DH are packed into D1out and DHout
bool ps_hpcp_update_step(const PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, double sigma, const PSMatrix& WH, PSMatrix& D1out,
                         PSMatrix& DHout, double* energy);
// Option complex_hpcp (one rank, inside a session that takes complex operands): ps_hpcp_traces, ps_hpcp_update and
// ps_hpcp_update_step take COMPLEX operands (slab_extra.hip k_hpcp_traces<double2> / k_hpcp_update<double2, .>: the traces sum the
// real parts of the diagonals in the order of the real pass; the update is the real kernel's chain on each part of an entry, the
// values and patterns of the vocabulary calls at threshold 0 bit for bit, *energy = Re dot(D1, WH) to rounding).  No collective.
// Gates (complex_hpcp off -- hpcp_step is for real operands only --, several ranks, no complex session, block or loose form, a
// labelled slab form, operands that are not all complex, of one dimension and distinct; in the loop: operands not left in slab
// form by the products; alignments that differ, a WH that becomes neither a zero-free slab form nor a read-only view) count
// nothing; past them a sigma that is zero or not finite, an operand the kernel's rules exclude once it is in slab form (stored
// zeros in a merged operand) and a non-zero status (runs far apart, an underflow) count as refused in complex_hpcp_counts().
// slab_algebra_counts() counts a fused pass as the real branch does; hpcp_step_counts() never counts a complex pass.
long long* complex_hpcp_counts();   // (slots: counters.inc)
// DIAGNOSTIC (the C ABI's ntpoly_amd_hpcp_traces_step): both matrices are brought into slab form where they are and the fused trace
// pass runs, real (option hpcp_step) or complex (option complex_hpcp); false: gated or refused, out as it was
bool ps_hpcp_traces_step(const PSMatrix& DDH, const PSMatrix& D2DH, double out[2]);
long long* hpcp_step_counts();   // (slots: counters.inc)
// ScaleAndFold (DensityMatrixSolversModule.F90:1049-1081) inside a real slab session, option scale_fold_step (slab_extra.hip
// k_saf_update / k_saf_dot_trace).
// ps_saf_update: what ps_axpby(X2, X, a, b, 0) -- ScaleMatrix(X, b); IncrementMatrix(X2, X, a) -- leaves in X, values and pattern bit
// for bit, *dot = dot(X, WH) of that X to rounding (another summation order; it only feeds the convergence monitor) and *trace =
// ps_trace of that X with its bits, from one pass and one read-back.  ps_saf_dot_trace: the same two numbers of X as it stands, one
// pass over X and WH.  Counted in slab_algebra_counts() as the calls replaced (the merge, the dot, the trace).
// Collective: past gates that are the same on every rank (the option off, no open real session, a complex operand, dimensions
// that differ, one matrix twice, block form) each rank enters ONE reduction of {dot, trace}; across ranks a rank whose panel is
// not taken runs the calls on it and adds the partial sums they compute, and the call still returns true.  false: nothing done
// (an operand still in compressed columns may have been turned into slab form) -- the caller makes the calls.  On one rank that
// is also the answer where the panel is not taken: by a gate of its own that counts nothing (a session that has given up slab
// form, a labelled slab form, every merged operand in compressed columns, alignments that differ, a WH that is neither a zero-free
// slab form nor a read-only view), or refused and counted so (a or b not finite, an operand the slab form cannot hold, runs far
// apart, a scaled entry that underflows to zero).
bool ps_saf_update(PSMatrix& X, const PSMatrix& X2, double a, double b, const PSMatrix& WH, double* dot, double* trace);
bool ps_saf_dot_trace(const PSMatrix& X, const PSMatrix& WH, double* dot, double* trace);
// DIAGNOSTICS (the C ABI's ntpoly_amd_scale_fold_update_step / _dot_trace): the operands are brought into slab form where they are,
// one pass runs, the new X is packed into Xout; false: refused or gated, everything as it was
bool ps_saf_update_step(const PSMatrix& X, const PSMatrix& X2, double a, double b, const PSMatrix& WH, PSMatrix& Xout, double* dot, double* trace);
bool ps_saf_dot_trace_step(const PSMatrix& X, const PSMatrix& WH, double* dot, double* trace);
long long* scale_fold_step_counts();   // (slots: counters.inc)
// The WOM solvers (FermiOperatorModule.F90:349-520) inside a real slab session, option wom_session = 2 (wom_heun.hip).
// ps_wom_heun: what CopyMatrix(W, RK2); IncrementMatrix(K0, RK2, step * 0.5, threshold); IncrementMatrix(K1, RK2, step * 0.5, threshold)
// leave in RK2, values and pattern bit for bit, *err = MatrixNorm of RK1 - RK2 and *err2 = MatrixNorm of RK2 - W (each difference
// merged at threshold) with the bits ps_norm gives on them in the session, from one pass and one read-back.  ps_wom_c_dots: out =
// {dot(X, W), dot(W, XA)} with the bits of two ps_dot calls in the session.  Counted in slab_algebra_counts() as the calls replaced
// (seven merges / copies and two norms; two dots).
// Collective: past gates that are the same on every rank (the option below 2, no open real session, a complex operand, block form,
// a labelled slab form, dimensions that differ, one matrix given twice) each rank enters ONE max-reduction of {err, err2} (ONE
// sum-reduction of the two dots); across ranks a rank whose panel is not taken builds its RK2 with the local merges, takes its two
// maxima from the local column sums, joins the reduction, and the call still returns true.  false: nothing done (an operand still
// in compressed columns may have been turned into slab form) -- the caller makes the calls.  On one rank that is also the answer
// where the pass is refused (counted so: step or threshold not finite, an operand the slab form cannot hold, alignments that
// differ, runs far apart, a kept value that is exactly zero).
bool ps_wom_heun(const PSMatrix& W, const PSMatrix& K0, const PSMatrix& K1, const PSMatrix& RK1, double step, double threshold, PSMatrix& RK2,
                 double* err, double* err2);
bool ps_wom_c_dots(const PSMatrix& X, const PSMatrix& W, const PSMatrix& XA, double out[2]);
// DIAGNOSTIC (the C ABI's ntpoly_amd_wom_heun_step): the same pass with RK2 packed into RK2out; false: refused or gated, everything as it was
bool ps_wom_heun_step(const PSMatrix& W, const PSMatrix& K0, const PSMatrix& K1, const PSMatrix& RK1, double step, double threshold,
                      PSMatrix& RK2out, double* err, double* err2);
long long* wom_session_counts();   // (slots: counters.inc)
// PurificationExtrapolate (GeometryOptimizationModule.F90:24-136) inside a real slab session, option purify_session = 2
// (purify_tail.hip).  ps_purify_tail: everything behind the iteration's two products in one pass and one read-back.  D = the
// working density, N = the product D S D, S = the working overlap.  fold: N becomes N' = 2 D - N, what ScaleMatrix(N, -1);
// IncrementMatrix(D, N, 2) leave, values and pattern bit for bit; otherwise N' = N stays the product's output.  *norm = MatrixNorm of
// D - N' (merged at threshold 0) and *next_trace = DotMatrix(N', S), each with the bits ps_norm / ps_dot give in the session.  D
// and S are only read.  Counted in slab_algebra_counts() as the calls replaced (fold: two merges, the copy, the scaling, the norm
// and the dot; plain: one merge, the copy, the norm and the dot).
// Collective: past gates that are the same on every rank (the option below 2, no open real session, a complex operand, block form,
// a labelled slab form, dimensions that differ, one matrix given twice) each rank enters ONE sum-reduction of the dot and ONE
// max-reduction of the norm; across ranks a rank whose panel is not taken builds its N' with the local calls, takes its parts
// from the local dot and column sums, joins the reductions, and the call still returns true.  false: nothing done (an operand
// still in compressed columns may have been turned into slab form) -- the caller makes the calls.  On one rank that is also the
// answer where the pass is refused (counted so: an operand the slab form cannot hold, a D or N that is a view, alignments that
// differ, runs far apart, an input that is not finite, a kept value that is exactly zero).
bool ps_purify_tail(const PSMatrix& D, PSMatrix& N, const PSMatrix& S, bool fold, double* norm, double* next_trace);
// DIAGNOSTIC (the C ABI's ntpoly_amd_purify_tail_step): the same pass with N' packed into Nout (plain: a copy of N); D, N and S keep
// their values.  One rank only (across ranks it is gated: no reduction is entered).  false: refused or gated, everything as it was
bool ps_purify_tail_step(const PSMatrix& D, const PSMatrix& N, const PSMatrix& S, bool fold, PSMatrix& Nout, double* norm, double* next_trace);
long long* purify_session_counts();   // (slots: counters.inc)
// ComputeExponentialPade (ExponentialSolversModule.F90:152-271) inside a real slab session, option pade_session = 2
// (pade_chain.hip).  ps_pade_chain: one of the call's two groups of merges in one pass and one read-back.  For q = 1, 2
//   Out_q = CopyMatrix(Base); ScaleMatrix(Out_q, scales[q - 1]); IncrementMatrix(*addends[k], Out_q, coeffs[(q - 1) n_addends + k], 0)
// for k = 0 .. n_addends - 1, n_addends 1 or 3, values and patterns bit for bit.  The inputs are only read (one still in compressed
// columns is turned into slab form where it is).  Counted in slab_algebra_counts() as the calls replaced.  Local: no reduction
// is entered, and the calls it replaces are local too, so across ranks each panel decides for itself.  false: nothing done --
// kept out by a gate (the option below 2, no open real session, a complex operand, block form, a labelled slab form, dimensions
// that differ, one matrix given twice, another n_addends: counted nowhere) or refused (counted so: an operand the slab form
// cannot hold or a view, alignments that differ, runs far apart, an input that is not finite, a scaled value that is exactly zero
// where an entry is held) -- the caller makes the calls.
bool ps_pade_chain(const PSMatrix& Base, const PSMatrix* const* addends, int n_addends, const double scales[2], const double* coeffs,
                   PSMatrix& Out1, PSMatrix& Out2);
// DIAGNOSTIC (the C ABI's ntpoly_amd_pade_chain_step): the same pass with both outputs packed.  One rank only (several ranks are a gate)
bool ps_pade_chain_step(const PSMatrix& Base, const PSMatrix* const* addends, int n_addends, const double scales[2], const double* coeffs,
                        PSMatrix& Out1, PSMatrix& Out2);
long long* pade_session_counts();   // (slots: counters.inc)
// solver_cg will run its loop in a slab session of its own on these operands (option cg_dots; the gate of its SlabSession).
// *dots: the loop takes its traces from column dot passes; *complex_session: that session takes complex operands.  solver_cg
// permutes its operands (a load balancer's permutation) BEFORE that session opens: a caller with such a permutation hands it
// compressed columns
bool solver_cg_opens_session(const PSMatrix& AMat, const PSMatrix& BMat, bool* dots = nullptr, bool* complex_session = nullptr);
// Option complex_scale_fold (one rank, inside a session that takes complex operands): the four calls above take COMPLEX operands
// (slab_extra.hip k_saf_update<double2, .>: the real kernel's scaling and merge on each part of an entry, the values and pattern of
// the vocabulary calls at threshold 0 bit for bit; the scale branch's pass is slab_dot_trace_c over X and WH as it stands -- slab
// form, a read-only view or compressed columns).  *dot = Re dot(X, WH) to rounding, *trace = the sum of the real parts of the
// diagonal with the bits of slab_dot_trace_c -- which, with the option on, is what ps_trace returns for a complex slab-form matrix
// in a complex session (trace_local; with the option at 0, and for compressed columns, k_trace as before).  No collective.  Gates (complex_scale_fold off -- scale_fold_step is for real
// operands only --, several ranks, no complex session, block or loose form, a labelled slab form, operands that are not all
// complex, of one dimension and distinct; in the loop: X not left in slab form by the product; alignments that differ, a WH that
// becomes neither a zero-free slab form nor a read-only view) count nothing; past them factors that are not finite, an operand the
// kernel's rules exclude once it is in slab form (stored zeros in a merged operand) and a non-zero status (runs far apart, an
// underflow) count as refused in complex_scale_fold_counts().  slab_algebra_counts() counts a fused pass as the real branch does;
// scale_fold_step_counts() never counts a complex pass.
long long* complex_scale_fold_counts();   // (slots: counters.inc)
// solvers.cpp: this loop may take a complex operand like m in slab form (FMA arithmetic, complex tile kernel, complex_sessions)
bool complex_slab_loop(const PSMatrix& m);
void ps_slab_leave(PSMatrix& m);   // back to compressed columns (no-op for a matrix that is not in slab form)
const long long* column_fused_counts();   // (slots: counters.inc)
const long long* block_algebra_counts();   // (slots: counters.inc)
long long block_scope_products();   // panel products of block-order solves that took the block path (psmatrix.cpp)
bool block_scope_active();   // band_scope.cpp: the solve in progress runs on operands redistributed in a block order (several ranks)
const long long* panel_product_counts();   // (slots: counters.inc)
long long recurrence_step_count();         // fused recurrence steps taken since start (each also counted as two merges below)
const long long* slab_algebra_counts();   // (slots: counters.inc)
void ps_fill_identity(PSMatrix& m);
void ps_fill_permutation(PSMatrix& m, const std::vector<int32_t>& lookup /*1-based*/, bool rows);
void ps_fill_from_triplets(PSMatrix& m, const HostTriplets& t);
void ps_get_triplets(const PSMatrix& m, HostTriplets& t);
int64_t ps_size(const PSMatrix& m);
// PSMatrixModule utilities on the caller side of the path (triplet based, as in the reference)
void ps_fill_dense(PSMatrix& m);                                          // FillMatrixDense: every element 1
void ps_diagonal_scale(PSMatrix& m, const HostTriplets& t);               // MatrixDiagonalScale: column col *= value
void ps_get_block(const PSMatrix& m, int sr, int er, int sc, int ec, HostTriplets& out);  // [sr,er) x [sc,ec), 1-based
void ps_get_slice(const PSMatrix& m, PSMatrix& sub, int sr, int er, int sc, int ec);      // inclusive bounds, 1-based
void ps_resize(PSMatrix& m, int new_size);
void ps_to_complex(const PSMatrix& a, PSMatrix& out);
void ps_to_real(const PSMatrix& a, PSMatrix& out);
void panel_exchange_layout(int32_t dim, int P, int me, const int64_t* req, const int64_t* cnt, int32_t* sa, int32_t* sb, int64_t* soff,
                           int32_t* ra, int32_t* rb, int64_t* zoff);   // psmatrix.cpp: who sends which columns where in a panel exchange (host)
DevMat ps_gather_full(const PSMatrix& m);  // every rank gets the whole matrix (dim x dim)
// range-restricted exchange: a dim x dim matrix holding only the columns [kmin, kmax] of the distributed matrix
// halo exchange for C = A*B: the columns of A named by the rows of the local B panel; also returns the global
// nnz of A and B (collected in the same exchange)
DevMat gather_needed(const PSMatrix& m, const DevMat& Bloc, int64_t nnz_global[2]);
// The same exchange in two steps, so that the caller can multiply the INTERIOR columns of its B panel (those that
// name only local columns of A) while the halo travels on the communication stream: begin() does the two size
// round trips and posts the send / recv group -- on comm_stream when `overlapped` comes back true --, finish() makes
// the engine stream wait for it and builds the column offsets of `full`.
struct HaloExchange {
  DevMat full;                    // dim x dim, columns outside the needed range empty; valid after finish()
  bool overlapped = false;
  int32_t kmin = 0, kmax = -1;    // columns of the distributed matrix present in `full` (the requested range)
  int32_t jl = 0, jr = 0;         // interior columns [jl, jr) of the local B panel (overlapped mode)
  int64_t off_l = 0, off_r = 0;   // their entry offsets in the panel
  // state between begin and finish
  DevBuf<int64_t> stage;
  std::vector<int32_t> ra, rb;
  std::vector<int64_t> zoff, soff, cnt_from;
  int32_t dim = 0;
  int P = 1;
  void finish();
};
void gather_needed_begin(HaloExchange& hx, const PSMatrix& m, const DevMat& Bloc, int64_t nnz_global[2], bool may_overlap);
void halo_segment(int32_t dim, int P, int s, int32_t kmin, int32_t kmax, int32_t* a, int32_t* b);
// concatenate the column panels of all ranks (widths[r] = columns held by rank r, known to all)
DevMat gather_panels(const DevMat& loc, const std::vector<int32_t>& widths);

// PSMatrixAlgebraModule
void ps_multiply(const PSMatrix& A, const PSMatrix& B, PSMatrix& C, double alpha, double beta, double threshold);
void ps_increment(const PSMatrix& A, PSMatrix& B, double alpha, double threshold);
void ps_scale(PSMatrix& A, double c);
void ps_axpby(const PSMatrix& A, PSMatrix& B, double alpha, double beta, double threshold);   // ScaleMatrix + IncrementMatrix, one pass
// B <- alpha*A + beta*B with the increment rules and, fused, out = dot(B_new, D) (TRS2 update + energy)
void ps_axpby_dot(const PSMatrix& A, PSMatrix& B, double alpha, double beta, double threshold, const PSMatrix& D, double out[4],
                  bool want_trace = false);  // out[2] = trace(B_new) on request
void ps_dot_trace(const PSMatrix& A, const PSMatrix& B, double out[4], bool want_trace);
void ps_square_dot(PSMatrix& B, PSMatrix& scratch, double threshold, const PSMatrix& D, double out[4], bool want_trace);
// a TRS2 solve starts: complex iterates try the complex slab form again (psmatrix.cpp complex_trs2_step)
void trs2_complex_reset();
// B <- 2B - B*B (threshold on the product and on the merge, TRS2's sigma > 0 update), out = dot(B_new, D), trace(B_new);
// the product goes from the numeric kernel's slots straight into the merge when the slab kernel computes it
void ps_square_update_dot(PSMatrix& B, PSMatrix& scratch, double threshold, const PSMatrix& D, double out[4], bool want_trace);
void ps_pairwise(const PSMatrix& A, const PSMatrix& B, PSMatrix& C);
void ps_dot(const PSMatrix& A, const PSMatrix& B, double out[2]);
double ps_trace(const PSMatrix& A);
double ps_norm(const PSMatrix& A);
double ps_sigma(const PSMatrix& A);
void ps_gershgorin(const PSMatrix& A, double* e_min, double* e_max);
void ps_transpose(const PSMatrix& A, PSMatrix& AT);
void ps_conjugate(PSMatrix& A);
// Option slab_transpose (>= 1), one rank without process slices, inside a slab session that takes the operand's kind: ps_transpose
// of a square zero-free slab form is the tiled transpose of its runs (kernels.hpp slab_transpose) and leaves a slab form, and
// ps_conjugate of a complex one runs in place.  A view, a labelled form or block form is gated: the path on compressed columns, A
// untouched, counted nowhere.  A transpose the pass refuses past the gates (extents far apart) runs on a packed copy of A, leaves
// compressed columns and counts as a refusal of the session.
long long* slab_transpose_counts();   // (slots: counters.inc)
// DIAGNOSTIC (the C ABI's ntpoly_amd_slab_transpose): one rank; a session of its own (a complex one where A is complex and FMA
// arithmetic, complex_tile and complex_sessions allow it), A entered into slab form, the pass run with or without conjugation, the
// PACKED result installed in AT.  false: gated or refused, AT untouched.  A is back in compressed columns either way
bool ps_slab_transpose_step(const PSMatrix& A, PSMatrix& AT, bool conj);
// PowerBounds on one vector (option power_vector; power_vector.hip).  The N columns of the reference's iterate are one vector and
// stay one vector, so the loop carries that column as a dense array on the device: x (the iterate), y = A x pruned as the product
// prunes, and the three sums of a step -- d1 = sum conj(x) x, d2 = Re sum conj(x) y, n1 = sum |y| -- in one read-back.
// ps_power_vector_open: the gate (no process slices; the option is the caller's) and the gather form of A, built from its
// compressed columns as ps_transpose takes them, A untouched.  Collective: false on EVERY rank when a gate holds or some rank
// could not build its form (32-bit indices, device memory).  Across ranks a rank's form holds the k of its own panel, a step sums
// the ranks' partial vectors through the transport and every rank prunes, reduces and scales the full vector identically.
// ps_power_vector_step: one step on pv.x; scale: x <- y / n1 behind it (ScaleMatrix's one multiplication); sums = (d1, d2, n1).
struct PowerVector {
  PowerGather G;
  DevBuf<double> x, y, part, out;
  int32_t n = 0;
  bool cplx = false, multi = false;
};
bool ps_power_vector_open(const PSMatrix& A, PowerVector& pv);
void ps_power_vector_set(PowerVector& pv, const double* host_x);   // n doubles, 2 n interleaved for a complex A
void ps_power_vector_step(PowerVector& pv, double threshold, bool scale, double sums[3]);
// DIAGNOSTIC (the C ABI's ntpoly_amd_power_vector_step): one unscaled step on a caller's x; y = the pruned product.  false:
// refused, nothing written.  Does not depend on the option and counts nothing
bool ps_power_vector_diag(const PSMatrix& A, const double* x, double* y, double threshold, double sums[3]);
long long* power_vector_counts();   // (slots: counters.inc)
// The traces of CGSolver from column dot passes (option cg_dots; cg_dots.hip k_cg_dots / k_cg_trace), inside a slab session.
// ps_cg_dots: out[0] = trace(prune(U1^H V1)), and with a second pair out[1] = trace(prune(U2^H V2)), pruned at `threshold` as
// MatrixMultiply prunes: what conj_transpose + ps_multiply(., ., ., 1, 0, threshold) + ps_trace give outside a session, bit for bit,
// without the transpose and without the product -- entry (j, j) of U^H V is the dot of column j of U with column j of V.  Operands
// still in compressed columns are brought into slab form where they are.  Collective as ps_hpcp_traces: past gates that are the
// same on every rank -- the option off, no open session for the operands' kind, block form, process slices > 1, complex operands
// with the option below 2 or on several ranks -- every rank enters ONE reduction of both sums; a rank whose panels the kernel does
// not take (an empty panel, operands that are not run-like, a labelled form) adds the same chains computed on its compressed columns
// (counted as refused).  false: gated, nothing done -- the caller runs transpose + product + trace.  Counted in
// slab_algebra_counts() as the operations it replaces: per pair a product, and a transpose and a trace as other operations.
bool ps_cg_dots(const PSMatrix& U1, const PSMatrix& V1, const PSMatrix* U2, const PSMatrix* V2, double threshold, double out[2]);
// DIAGNOSTIC (the C ABI's ntpoly_amd_cg_dots): a session of its own for the operands' kind, both operands into slab form, one pass
// with one pair -- k_cg_dots, or for operands without a slab form (not run-like, an empty panel) the chains on compressed columns,
// as in the loop; diag = the d_j of the local columns (U.c1 - U.c0 doubles), *trace = their sum over all ranks.  false: gated,
// nothing written.  Under the option's gates (real operands: 1, complex ones: 2, one rank); counts nothing
bool ps_cg_dots_diag(const PSMatrix& U, const PSMatrix& V, double threshold, double* diag, double* trace);
long long* cg_dots_counts();   // (slots: counters.inc)
bool ps_is_identity(const PSMatrix& A);
double ps_measure_asymmetry(const PSMatrix& A);
void ps_symmetrize(PSMatrix& A);
void ps_similarity(const PSMatrix& A, const PSMatrix& P, const PSMatrix& PInv, PSMatrix& Res, double threshold);
// LoadBalancerModule
struct Permutation {
  std::vector<int32_t> index_lookup, reverse_index_lookup;  // 1-based values
};
void permutation_default(Permutation& p, int n);
void permutation_reverse(Permutation& p, int n);
void permutation_random(Permutation& p, int n);
void ps_permute(const PSMatrix& in, PSMatrix& out, const Permutation& perm, bool undo);

// ------------------------------------------------------------------ logger (LoggingModule.F90)
struct Logger {
  bool active = false;
  int level = 0;
  FILE* out = stdout;
  bool owns_file = false;
};
Logger& logger();
void log_activate(bool start_document, const char* file_name);
void log_deactivate();
void log_enter();
void log_exit();
void log_header(const char* h);
void log_element(const char* key, double v);
void log_element(const char* key, int v);
void log_element(const char* key, const char* v);
void log_element(const char* key, bool v);
void log_list_element(const char* key, double v);
void log_list_element(const char* key);

// ------------------------------------------------------------------ solver parameters / monitor
struct Monitor {  // ConvergenceMonitorModule.F90:14-27
  double win_short[3] = {0, 0, 0}, win_long[6] = {0, 0, 0, 0, 0, 0};
  int nval = 0;
  double loose_cutoff = 1e-2, tight_cutoff = 1e-8;
  bool automatic = true;
};
void monitor_construct(Monitor& m, bool automatic, double tight_cutoff);
void monitor_append(Monitor& m, double v);
bool monitor_converged(const Monitor& m, bool be_verbose);

struct SolverParameters {  // SolverParametersModule.F90:14-33, defaults :48-50
  double converge_diff = 1e-6;
  int max_iterations = 1000;
  double threshold = 0.0;
  bool be_verbose = false;
  bool do_load_balancing = false;
  Permutation balance_permutation;
  double step_thresh = 1e-2;
  bool monitor_convergence = true;
};
void print_parameters(const SolverParameters& p);
void print_matrix_information(const PSMatrix& m);
// what the solvers share around their loops (solvers.cpp).  solver_header, when p is verbose: the title, one level in, the
// Method if there is one, the "Citations" block and the parameters; the caller's last log_exit closes it.  The balance_*
// calls act under p.do_load_balancing only: m under p's permutation, in place; out = `in` under it (a plain copy
// without load balancing); m back under the caller's labels
void log_citations(std::initializer_list<const char*> keys);
void solver_header(const char* title, const char* citation, const SolverParameters& p, const char* method = nullptr);
void balance_permute(PSMatrix& m, const SolverParameters& p);
void balance_copy(const PSMatrix& in, PSMatrix& out, const SolverParameters& p);
void balance_undo(PSMatrix& m, const SolverParameters& p);

// per-iteration record of the last solver call (tests/bench read it through the C ABI extension)
struct SolverTrace {
  std::vector<double> value, energy, sigma;
  std::vector<int64_t> nnz;
  int iterations = 0;
  double setup_ms = 0, loop_ms = 0;
};
SolverTrace& last_trace();
// matrix polynomials (solvers_poly.cpp): coefficient i of the vector multiplies x^i / T_i(x) / H_i(x)
void polynomial_horner(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p);
void polynomial_paterson_stockmeyer(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p);
// (keep_slab_form, internal: Out stays in the slab form the evaluation's session left it in -- for compute_exponential, whose own
// session is open around the call and squares Out next; never with a load balancer's permutation, which is undone on compressed
// columns.  The C ABI packs as ever)
void chebyshev_compute(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p, bool keep_slab_form = false);
void chebyshev_factorized(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p);
void hermite_compute(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p);
// matrix functions (solvers_func.cpp)
void power_bounds(const PSMatrix& A, double* max_value, const SolverParameters& p, bool defaults);
void compute_exponential(const PSMatrix& In, PSMatrix& Out, const SolverParameters& p);
void compute_logarithm(const PSMatrix& In, PSMatrix& Out, const SolverParameters& p);
void compute_sine(const PSMatrix& In, PSMatrix& Out, const SolverParameters& p);
void compute_cosine(const PSMatrix& In, PSMatrix& Out, const SolverParameters& p);
void compute_root(const PSMatrix& In, PSMatrix& Out, int root, const SolverParameters& p);
void compute_inverse_root(const PSMatrix& In, PSMatrix& Out, int root, const SolverParameters& p);
// DensityMatrixSolversModule.F90:953-1117, :1165-1187, :1190-1231
void solver_scale_and_fold(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double homo, double lumo,
                           double* energy_out, const SolverParameters& p);
void energy_density_matrix(const PSMatrix& H, const PSMatrix& D, PSMatrix& ED, double threshold);
void mcweeny_step(const PSMatrix& D, PSMatrix& DOut, const PSMatrix* S, double threshold);
// one TRS2 iteration (DensityMatrixSolversModule.F90:380-404): returns the energy, sets sigma
double trs2_step(PSMatrix& X, PSMatrix& X2, const PSMatrix& WH, double trace_target, double threshold, double* sigma,
                 double* trace_io = nullptr);

// band_scope.cpp: a solver on several ranks whose first operand hides a band under its labels runs on operands redistributed
// in the recovered order (collective; false: not applicable -- the caller solves as it stands).  run(ins, outs) is the
// solver itself on the relabelled operands; the outputs are carried back to the caller's labels
bool band_scope_try(const std::vector<const PSMatrix*>& ins, const std::vector<PSMatrix*>& outs,
                    const std::function<void(const std::vector<const PSMatrix*>&, const std::vector<PSMatrix*>&)>& run);
const long long* band_scope_counts();   // (slots [0..1]: counters.inc; [2] solves that ran in a block order across ranks)

// ------------------------------------------------------------------ solvers
void solver_trs2(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy, double* mu,
                 const SolverParameters& p);
void solver_trs4(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy, double* mu,
                 const SolverParameters& p);
void solver_pm(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy, double* mu,
               const SolverParameters& p);
void solver_hpcp(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy, double* mu,
                 const SolverParameters& p);
void solver_sign(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p);
void solver_polar(const PSMatrix& A, PSMatrix& U, PSMatrix* Hm, const SolverParameters& p);
void solver_invert(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p);
void solver_pseudoinverse(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p);
void solver_square_root(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p, bool inverse, int order);

// solvers_extra.cpp: linear solvers, Pade exponential, geometry extrapolation, the dense (eigendecomposition) family,
// Fermi-operator solvers, Cholesky factorisations
void ps_filter(PSMatrix& m, double threshold);
void ps_gather_triplets(const PSMatrix& m, HostTriplets& t);
void solver_cg(const PSMatrix& A, PSMatrix& X, const PSMatrix& B, const SolverParameters& p);
void compute_exponential_pade(const PSMatrix& In, PSMatrix& Out, const SolverParameters& p);
void purification_extrapolate(const PSMatrix& PreviousDensity, const PSMatrix& Overlap, double trace, PSMatrix& NewDensity,
                              const SolverParameters& p);
void lowdin_extrapolate(const PSMatrix& PreviousDensity, const PSMatrix& OldOverlap, const PSMatrix& NewOverlap,
                        PSMatrix& NewDensity, const SolverParameters& p);
void snap_to_sparsity_pattern(PSMatrix& mat, const PSMatrix& pattern);
void ps_eigendecomposition(const PSMatrix& A, PSMatrix& eigenvalues, PSMatrix* eigenvectors, int nvals,
                           const SolverParameters& p);
void dense_matrix_function(const PSMatrix& A, PSMatrix& Result, const std::function<double(double)>& func,
                           const SolverParameters& p);
void ps_svd(const PSMatrix& A, PSMatrix& left, PSMatrix& right, PSMatrix& singular, const SolverParameters& p);
void estimate_gap(const PSMatrix& H, const PSMatrix& K, double chemical_potential, double* gap, const SolverParameters& p);
void compute_dense_foe(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, const double* inv_temp_in,
                       double* energy_out, double* mu_out, const SolverParameters& p);
void solver_wom(const PSMatrix& H, const PSMatrix& ISQ, PSMatrix& K, double inv_temp, const double* trace_in,
                const double* mu_in, double* energy_out, const SolverParameters& p);
void ps_cholesky(const PSMatrix& A, PSMatrix& L, int rank, const SolverParameters& p);
void reduce_dimension(const PSMatrix& A, int dim, PSMatrix& Reduced, const SolverParameters& p);

}  // namespace ntp
