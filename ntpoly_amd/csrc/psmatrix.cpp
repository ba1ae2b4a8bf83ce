// Distributed matrix (Matrix_ps) and distributed algebra on column panels.
// Reference: PSMatrixModule.F90, PSMatrixAlgebraModule.F90, ProcessGridModule.F90,
// LoadBalancerModule.F90, PermutationModule.F90.
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <numeric>
#include <optional>
#include <random>

#include "engine.hpp"
#include "spgemm_block.hpp"

namespace ntp {

namespace {
// non-owning window on the arrays of another DevMat: a column range of it, or the same entries under another
// column-offset array.  The kernels only ever index inner / val through the (absolute) offsets in `outer`.
struct MatView {
  DevMat m;
  void alias(const DevMat& src, int64_t* outer, int32_t cols, int64_t nnz) {
    m.rows = src.rows;
    m.cols = cols;
    m.cplx = src.cplx;
    m.nnz = nnz;
    m.outer.p = outer;
    m.inner.p = src.inner.p;
    m.val.p = src.val.p;
  }
  ~MatView() { m.outer.p = nullptr; m.inner.p = nullptr; m.val.p = nullptr; }
};
}  // namespace

// ------------------------------------------------------------------ process grid
namespace {
ProcessGrid g_grid;
bool g_grid_built = false;
}  // namespace
ProcessGrid& global_grid() { return g_grid; }
bool global_grid_constructed() { return g_grid_built; }

void construct_grid(ProcessGrid& g, int rows, int cols, int slices, Comm& c) {
  // grid sanity check (ProcessGridModule.F90:162-176): fatal if the shape does not match
  if (rows * cols * slices != c.nranks && !options().virtual_grid)
    NTP_FATAL("process grid " + std::to_string(rows) + "x" + std::to_string(cols) + "x" + std::to_string(slices) +
              " does not match " + std::to_string(c.nranks) + " processes");
  g.num_rows = rows;
  g.num_cols = cols;
  g.num_slices = slices;
  g.total = c.nranks;
  g.global_rank = c.rank;
  g.comm = &c == &base_world() ? nullptr : &c;
  // rank -> (slice, row, column) as ProcessGridModule.F90:180-183
  const int slice_size = rows * cols;
  g.my_slice = c.rank / slice_size;
  const int in_slice = c.rank - slice_size * g.my_slice;
  g.my_row = in_slice / cols;
  g.my_col = in_slice % cols;
  if (&g == &g_grid) g_grid_built = true;
}

void construct_grid_default(ProcessGrid& g, int slices, Comm& c) {
  // ComputeGridSize (ProcessGridModule.F90:576-601): most square rows x cols for the given slices
  const int total = c.nranks;
  if (slices <= 0) slices = 1;
  while (total % slices != 0) --slices;
  const int slice_size = total / slices;
  int rows = 1, cols = slice_size;
  for (int r = (int)std::floor(std::sqrt((double)slice_size)); r >= 1; --r) {
    if (slice_size % r == 0) {
      rows = r;
      cols = slice_size / r;
      break;
    }
  }
  construct_grid(g, rows, cols, slices, c);
}

ProcessGrid* split_process_grid(const ProcessGrid& old_grid, int* my_color, bool* split_slice) {
  static std::vector<ProcessGrid*>* kept = new std::vector<ProcessGrid*>();   // (grids made here live as long as the library)
  CommScope cs(&old_grid);
  int rows = 1, cols = 1, slices = 1, color = 0;
  *split_slice = false;
  if (old_grid.total == 1) {
    // base case (:447-453)
  } else if (old_grid.num_slices > 1) {          // preferably along the slices (:455-468)
    const int mid = old_grid.num_slices / 2;
    rows = old_grid.num_rows;
    cols = old_grid.num_cols;
    color = old_grid.my_slice < mid ? 0 : 1;
    slices = color == 0 ? mid : old_grid.num_slices - mid;
    *split_slice = true;
  } else if (old_grid.num_rows > old_grid.num_cols) {   // else the longer direction (:470-482)
    const int mid = old_grid.num_rows / 2;
    cols = old_grid.num_cols;
    color = old_grid.my_row < mid ? 0 : 1;
    rows = color == 0 ? mid : old_grid.num_rows - mid;
  } else {                                       // default: the columns (:484-496)
    const int mid = old_grid.num_cols / 2;
    rows = old_grid.num_rows;
    color = old_grid.my_col < mid ? 0 : 1;
    cols = color == 0 ? mid : old_grid.num_cols - mid;
  }
  *my_color = color;
  // MPI_COMM_SPLIT(global_comm, my_color, global_rank) (:499-501): the processes of a colour in the order of their old ranks
  Comm* nc = comm_split(color, old_grid.global_rank);
  auto* g = new ProcessGrid();
  kept->push_back(g);
  construct_grid(*g, rows, cols, slices, *nc);
  return g;
}

void ps_comm_split(const PSMatrix& m, PSMatrix& split, int* my_color, bool* split_slice) {
  const ProcessGrid& g = *m.grid;
  CommScope cs(&g);
  if (g.total == 1) {   // (distributed_includes/CommSplitMatrix.f90:11-14)
    ps_copy(m, split);
    *my_color = 0;
    *split_slice = true;
    return;
  }
  // every process of either half ends up with a share of the WHOLE matrix (:20-60: the triplets of the other half travel over
  // the between-grid communicator); here: the panels gathered once over the old grid, each process cuts the column panel it
  // owns on its half
  DevMat full = ps_gather_full(m);
  ProcessGrid* ng = split_process_grid(g, my_color, split_slice);
  ps_construct_empty(split, m.dim, ng, m.cplx);   // (the half's panel: on the half's communicator)
  split.loc = column_slice(full, split.c0, split.c1);
  sync_stream();
}

void write_grid_info(const ProcessGrid& g) {
  log_header("Process Grid");
  log_enter();
  log_element("Process Rows", g.num_rows);
  log_element("Process Columns", g.num_cols);
  log_element("Process Slices", g.num_slices);
  log_element("Column Panels (GPUs)", g.total);
  log_exit();
}

// ------------------------------------------------------------------ construction / fill
void panel_range(int32_t dim, int nranks, int rank, int32_t* c0, int32_t* c1) {
  *c0 = (int32_t)(((int64_t)dim * rank) / nranks);
  *c1 = (int32_t)(((int64_t)dim * (rank + 1)) / nranks);
}

// The layout of one panel exchange on rank `me`, from what every rank knows after the step's all-gather: req[4 q ..] = (first,
// last row of rank q's panel of B, ...), cnt[s P + q] = doubles rank s sends to rank q.  sa / sb [q]: my columns [sa, sb) go to
// rank q, packed from soff[q] in my send buffer; ra / rb [s]: the columns [ra, rb) of rank s arrive at zoff[s] of my receive
// buffer (nothing travels from a rank to itself).  Pure host arithmetic (tests/test_distributed_cpu.py drives it over gloo).
namespace {
// the rows [kmin, kmax] that rank q's request names (an empty panel: kmax < kmin)
int32_t req_kmin(const int64_t* req, int q) { const int64_t lo = req[(size_t)4 * q], hi = req[(size_t)4 * q + 1]; return hi < lo ? 0 : (int32_t)lo; }
int32_t req_kmax(const int64_t* req, int q) { const int64_t lo = req[(size_t)4 * q], hi = req[(size_t)4 * q + 1]; return hi < lo ? -1 : (int32_t)hi; }
}  // namespace
void panel_exchange_layout(int32_t dim, int P, int me, const int64_t* req, const int64_t* cnt, int32_t* sa, int32_t* sb, int64_t* soff,
                           int32_t* ra, int32_t* rb, int64_t* zoff) {
  soff[0] = 0;
  zoff[0] = 0;
  for (int q = 0; q < P; ++q) {
    halo_segment(dim, P, me, req_kmin(req, q), req_kmax(req, q), &sa[q], &sb[q]);
    soff[q + 1] = soff[q] + (q == me ? 0 : cnt[(size_t)me * P + q]);
  }
  for (int s = 0; s < P; ++s) {
    halo_segment(dim, P, s, req_kmin(req, me), req_kmax(req, me), &ra[s], &rb[s]);
    zoff[s + 1] = zoff[s] + (s == me ? 0 : cnt[(size_t)s * P + me]);
  }
}

void ps_construct_empty(PSMatrix& m, int32_t dim, const ProcessGrid* g, bool cplx) {
  if (!g) NTP_FATAL("matrix constructed without a process grid (construct the global grid first)");
  ensure_init();
  CommScope cs(g);   // (the matrix lives on its grid's communicator: its panel is one of that communicator's)
  m.grid = g;
  m.dim = dim;
  m.cplx = cplx;
  panel_range(dim, world().nranks, world().rank, &m.c0, &m.c1);
  m.loc.reset_empty(dim, m.c1 - m.c0, cplx);
}

void ps_construct_like(PSMatrix& m, const PSMatrix& ref) { ps_construct_empty(m, ref.dim, ref.grid, ref.cplx); }

namespace {
// the header and the local panel of a result
void install(PSMatrix& X, const ProcessGrid* grid, int32_t dim, bool cplx, int32_t c0, int32_t c1, DevMat&& loc) {
  X.grid = grid; X.dim = dim; X.cplx = cplx; X.c0 = c0; X.c1 = c1;
  X.loc = std::move(loc);
}
// dense-branch rule of the local multiply (GemmMatrix.f90:49-61) from the operands' entry counts; a_fraction: the share of the
// inner dimension A is populated over (multiply_panel)
bool dense_branch(int32_t dim, int64_t nnz_a, int64_t nnz_b, double a_fraction = 1.0) {
  const double denom = (double)dim * (double)dim;
  return denom > 0 && std::min((double)nnz_a / (denom * a_fraction), (double)nnz_b / denom) > 0.1;
}
bool beta_is_zero(double beta) { return std::fabs(beta) < 2.2250738585072014e-308; }
int g_slab_depth = 0;
bool g_slab_failed = false;
bool slab_on() { return g_slab_depth > 0 && !g_slab_failed; }
// (the representation of an operand, not its value, changes: const operands are converted in place)
DevMat& mut(const PSMatrix& m) { return const_cast<DevMat&>(m.loc); }
int g_slab_refusals = 0;
bool g_complex_session = false;   // the open session's loop takes complex operands in slab form (SlabSession complex_ok)
bool g_keep_sparse_runs = false;  // the open session's products stay on the register-slab kernel in unfused arithmetic (slab_keep_sparse_runs)
long long g_recurrence_steps = 0;   // fused recurrence steps taken (ps_recurrence_step returned true)
long long g_slab_counts[4] = {0, 0, 0, 0};   // products, merges / copies, other operations in slab form; refusals
// the slab algebra of one element kind, for the operations that exist for both (kernels.hpp: name, name_c)
struct SlabKind {
  bool (*enter)(DevMat&);
  bool (*multiply)(const DevMat&, const DevMat&, DevMat&, double, double, bool, const SlabHalo*);
  bool (*takes_panel)(const DevMat&, const DevMat&, int, int32_t, int32_t, const SlabPlan*);
  bool (*clone)(const DevMat&, DevMat&);
  bool (*scale)(DevMat&, double);
  bool (*axpby)(const DevMat&, DevMat&, double, double, double);
  bool (*axpby_to)(const DevMat&, const DevMat&, DevMat&, double, double, double);
  bool (*add_diagonal)(DevMat&, double, int32_t);
  bool (*norm)(const DevMat&, double*);
  bool (*norm_axpby)(const DevMat&, const DevMat&, double, double, double*);
};
const SlabKind& slab_kind(bool cplx) {
  static const SlabKind kinds[2] = {
      {slab_enter, slab_multiply, slab_multiply_takes_panel, slab_clone, slab_scale, slab_axpby, slab_axpby_to, slab_add_diagonal, slab_norm,
       slab_norm_axpby},
      {[](DevMat& M) { return slab_enter_c(M); }, slab_multiply_c, slab_multiply_c_takes_panel, slab_clone_c, slab_scale_c, slab_axpby_c,
       slab_axpby_to_c, slab_add_diagonal_c, slab_norm_c, slab_norm_axpby_c}};
  return kinds[cplx ? 1 : 0];
}
// this session takes operands of this kind in slab form
bool session_takes(bool cplx) { return !cplx || g_complex_session; }
// an operation that cannot be done in slab form: its operands go back to compressed columns and the general path does
// it (a Hamiltonian with stored zeros in the first merge of a loop); the session goes on, unless this keeps happening
void slab_refused(std::initializer_list<const PSMatrix*> ms) {
  g_slab_refusals += 1;
  g_slab_counts[3] += 1;
  if (g_slab_refusals > 4) g_slab_failed = true;
  if (std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
    std::fprintf(stderr, "[slab session] an operation was refused (%d so far)%s\n", g_slab_refusals,
                 g_slab_failed ? ": compressed columns from here on" : "");
  for (const PSMatrix* m : ms) pack(mut(*m));
}
// a read-only slab view of a matrix with stored zeros (SlabForm::origin, option stored_zero_views)
bool is_view(const PSMatrix& m) { return m.loc.expanded() && m.loc.slab->origin != nullptr; }
void count_view_product(const PSMatrix& A, const PSMatrix& B) {
  if (is_view(A) || is_view(B)) slab_view_counts()[1] += 1;
}
// the compressed columns of an operand for ONE operation that the slab form cannot do: a view's own (no copy), otherwise a
// packed copy in `tmp` -- the operand itself stays in slab form
const DevMat& columns_of(const PSMatrix& m, DevMat& tmp) {
  if (is_view(m)) return *m.loc.slab->origin;
  if (!m.loc.expanded() && !m.loc.loose() && !m.loc.blocked()) return m.loc;
  tmp = packed_copy(m.loc);
  return tmp;
}
// A merge on a view was declined because its result has to STORE a zero (kernels.hip k_sa_axpby, stat bit 4): a refusal like
// any other in the session's books, but nobody loses its slab form over it -- the caller does this one merge on compressed
// columns (columns_of) and the view stands for the next product
void slab_refused_view_merge() {
  g_slab_refusals += 1;
  g_slab_counts[3] += 1;
  if (g_slab_refusals > 4) g_slab_failed = true;
  if (std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
    std::fprintf(stderr, "[slab session] a merge on a view keeps a stored zero: this one on compressed columns (%d refusals so far)\n", g_slab_refusals);
}
// Block form (DevMat::blk: what the block path's products leave behind for the C ABI's MatrixMultiply and the TRS2 loop)
// is understood by ps_multiply and the TRS2 steps only: every other operation takes compressed columns
void unblock(std::initializer_list<const PSMatrix*> ms) {
  for (const PSMatrix* m : ms)
    if (m->loc.blocked()) pack(mut(*m));
}
// the block algebra (spgemm_block.hpp) takes an operation when an operand is in block form (one rank)
bool blk_any(std::initializer_list<const PSMatrix*> ms) {
  if (world().active()) return false;
  for (const PSMatrix* m : ms)
    if (m->loc.blocked()) return true;
  return false;
}
// a slab form under a relabelling (a relabelled band): the fused passes walk rows in the caller's order and leave it alone
bool labelled(const PSMatrix& M) { return M.loc.expanded() && M.loc.slab->labelled(); }
// no matrix is named twice
bool all_distinct(std::initializer_list<const PSMatrix*> ms) {
  for (auto a = ms.begin(); a != ms.end(); ++a)
    for (auto b = a + 1; b != ms.end(); ++b)
      if (*a == *b) return false;
  return true;
}
bool same_dim(std::initializer_list<const PSMatrix*> ms) {
  for (const PSMatrix* m : ms)
    if (m->dim != (*ms.begin())->dim) return false;
  return true;
}
// install with the header of X (read before the move: Out may be X)
void install_like(PSMatrix& Out, const PSMatrix& X, bool cplx, DevMat&& loc) {
  const ProcessGrid* grid = X.grid;
  const int32_t dim = X.dim, c0 = X.c0, c1 = X.c1;
  install(Out, grid, dim, cplx, c0, c1, std::move(loc));
}
// complex operands stay in block form (complex products and the complex block algebra, spgemm_block.hpp) inside a session on
// one rank where complex sessions and the complex block path are both allowed -- a solver's complex session or a one-call
// session of the C ABI
bool complex_blocks_on() {
  return slab_on() && !world().active() && options().complex_sessions != 0 && options().spgemm_fma == 1 && options().complex_tile != 0 &&
         options().block_complex != 0 && options().block_path != 0;
}
// operands the block algebra may take together: both real, or mixed / complex with a complex one in block form (a real
// operand in compressed columns joins it as a complex form)
bool blk_kinds(const PSMatrix& A, const PSMatrix& B) {
  return (!A.cplx && !B.cplx) || (A.cplx && A.loc.blocked()) || (B.cplx && B.loc.blocked());
}
long long g_column_fused[2] = {0, 0};   // in-place identity increments, norms of differences (column_fused.hip)
long long g_block_counts[2] = {0, 0};   // operations of the block algebra; fallbacks to compressed columns
// an operation outside the session, or after a refusal: no operand may stay in slab form
void slab_pack_if(std::initializer_list<const PSMatrix*> ms) {
  if (g_slab_depth == 0) return;   // (outside a session nothing is left in slab form by one)
  for (const PSMatrix* m : ms)
    if (m->loc.expanded() || m->loc.loose() || m->loc.blocked()) pack(mut(*m));
}
}  // namespace

const long long* slab_algebra_counts() { return g_slab_counts; }
long long recurrence_step_count() { return g_recurrence_steps; }
const long long* block_algebra_counts() { return g_block_counts; }
const long long* column_fused_counts() { return g_column_fused; }

SlabSession::SlabSession(bool eligible, bool api, bool complex_ok) {
  // (more than one rank: the loops' matrices are column panels in slab form, a product exchanges the runs of its left
  // operand's halo -- panel_slab_multiply below; FMA arithmetic, real, the solvers' own sessions only: option panel_sessions)
  const bool multi = world().active();
  opened = eligible && options().slab_algebra != 0 && (options().spgemm_fma == 1 || options().spgemm_fma == 0) && options().spgemm_variant < 0 &&
           options().spgemm_force_bin <= 0 && (!multi || (options().panel_sessions != 0 && options().spgemm_fma == 1 && !api));
  if (opened && multi && g_slab_depth == 0) slab_allow_panels(true);
  // (complex loops across ranks: complex column panels in slab form, products on the complex tile kernel -- option complex_panels,
  // on top of what opened the panel session above)
  if (opened && complex_ok && options().complex_sessions != 0 && options().spgemm_fma == 1 && options().complex_tile != 0 && !g_complex_session &&
      (!multi || options().complex_panels != 0)) {
    g_complex_session = true;
    set_complex = true;
  }
  // (a one-call session of the C ABI on a matrix that is not run-like pays the refused conversion once: slab_enter leaves a
  // mark on the matrix, DevMat::slab_hint, and says no at once when asked again)
  if (opened) {
    if (g_slab_depth == 0) { g_slab_failed = false; g_slab_refusals = 0; }
    g_slab_depth += 1;
  }
}
SlabSession::~SlabSession() { close(); }
void SlabSession::close() {
  if (set_complex) { g_complex_session = false; set_complex = false; }
  if (opened) {
    g_slab_depth -= 1;
    if (g_slab_depth == 0) { slab_allow_panels(false); g_keep_sparse_runs = false; }
  }
  opened = false;
}
void slab_keep_sparse_runs(bool on) {
  if (g_slab_depth > 0) g_keep_sparse_runs = on;
}
void ps_slab_leave(PSMatrix& m) {
  if (m.loc.expanded() || m.loc.blocked()) pack(m.loc);
  drop_pending_exchange();   // (the iterate leaves slab form: no step follows the last one)
}

void ps_copy(const PSMatrix& a, PSMatrix& b) {
  CommScope cs(a.grid);
  if (&a == &b) return;
  if (blk_any({&a})) {
    DevMat t;
    if (block_clone(a.loc, t)) {
      g_block_counts[0] += 1;
      install(b, a.grid, a.dim, a.cplx, a.c0, a.c1, std::move(t));
      return;
    }
    g_block_counts[1] += 1;
  }
  unblock({&a});
  if (slab_on() && a.loc.expanded()) {
    // (a complex operand outside a session that takes them is refused: the real slab_clone declines it untouched)
    DevMat t;
    if (session_takes(a.cplx) && slab_kind(a.cplx).clone(a.loc, t)) {
      g_slab_counts[1] += 1;
      install(b, a.grid, a.dim, a.cplx, a.c0, a.c1, std::move(t));
      return;
    }
    slab_refused({&a});
  }
  install(b, a.grid, a.dim, a.cplx, a.c0, a.c1, a.loc.clone());
}

void ps_fill_identity(PSMatrix& m) {
  CommScope cs(m.grid);  // FillMatrixIdentity (O(N) here, O(N^2/P) in the reference)
  m.loc = identity(m.dim, m.c0, m.c1 - m.c0, m.cplx);
}

void ps_fill_permutation(PSMatrix& m, const std::vector<int32_t>& lookup, bool rows) {
  CommScope cs(m.grid);
  // distributed_includes/FillMatrixPermutation.f90:1-35
  HostTriplets t;
  t.cplx = m.cplx;
  const size_t w = m.cplx ? 2 : 1;
  for (int32_t ii = 1; ii <= m.dim; ++ii) {
    const int32_t col = rows ? lookup[(size_t)ii - 1] : ii;
    const int32_t row = rows ? ii : lookup[(size_t)ii - 1];
    if (col - 1 >= m.c0 && col - 1 < m.c1) {
      t.col.push_back(col);
      t.row.push_back(row);
      t.val.push_back(1.0);
      if (w == 2) t.val.push_back(0.0);
    }
  }
  m.loc = from_triplets(t, m.dim, m.c1 - m.c0, m.c0);
}

void ps_fill_from_triplets(PSMatrix& m, const HostTriplets& t) {
  CommScope cs(m.grid);
  // FillMatrixFromTripletList (distributed_includes/FillMatrixFromTripletList.f90:14-47): any rank
  // may hold any triplet.  Ranks exchange what they hold (setup path, host triplets travel through
  // device buffers because RCCL moves device memory) and keep their own columns.
  if (t.cplx != m.cplx) {
    HostTriplets conv;
    conv.cplx = m.cplx;
    conv.col = t.col;
    conv.row = t.row;
    if (m.cplx) {
      conv.val.resize(t.size() * 2);
      for (size_t i = 0; i < t.size(); ++i) {
        conv.val[2 * i] = t.val[i];
        conv.val[2 * i + 1] = 0.0;
      }
    } else {
      conv.val.resize(t.size());
      for (size_t i = 0; i < t.size(); ++i) conv.val[i] = t.val[2 * i];
    }
    ps_fill_from_triplets(m, conv);
    return;
  }
  for (size_t i = 0; i < t.size(); ++i)
    if (t.col[i] < 1 || t.col[i] > m.dim)
      NTP_FATAL("triplet " + std::to_string(i) + " names column " + std::to_string(t.col[i]) + " of a matrix of dimension " +
                std::to_string(m.dim));
  if (!world().active()) {
    m.loc = from_triplets(t, m.dim, m.c1 - m.c0, m.c0);
    return;
  }
  // multi-rank: every rank turns what it holds into a full-width matrix, all of them are gathered
  // (one grouped broadcast per rank) and each rank sums the pieces that fall into its own panel.
  // Contributions of different ranks are disjoint by contract.
  const int P = world().nranks;
  DevMat mine = from_triplets(t, m.dim, m.dim, 0);
  std::vector<int32_t> widths((size_t)P, m.dim);
  DevMat all = gather_panels(mine, widths);  // dim x (P*dim), rank r's matrix at columns [r*dim, (r+1)*dim)
  DevMat acc;
  acc.reset_empty(m.dim, m.c1 - m.c0, m.cplx);
  for (int r = 0; r < P; ++r) {
    DevMat part = column_slice(all, r * m.dim + m.c0, r * m.dim + m.c1);
    if (part.nnz) increment(part, acc, 1.0, 0.0);
  }
  m.loc = std::move(acc);
}

void ps_get_triplets(const PSMatrix& m, HostTriplets& t) {
  CommScope cs(m.grid); to_triplets(m.loc, m.c0, t); }

// FillMatrixDense (PSMatrixModule.F90:958-990, distributed_includes/FillMatrixDense.f90): every element of the
// local panel is 1; dense by definition, so the O(dim * width) host triplets are what the caller asked for
void ps_fill_dense(PSMatrix& m) {
  CommScope cs(m.grid);
  HostTriplets t;
  t.cplx = m.cplx;
  const size_t w = m.cplx ? 2 : 1;
  const size_t n = (size_t)m.dim * (size_t)(m.c1 - m.c0);
  t.col.reserve(n); t.row.reserve(n); t.val.reserve(n * w);
  for (int32_t c = m.c0; c < m.c1; ++c)
    for (int32_t r = 0; r < m.dim; ++r) {
      t.col.push_back(c + 1);
      t.row.push_back(r + 1);
      t.val.push_back(1.0);
      if (m.cplx) t.val.push_back(0.0);
    }
  m.loc = from_triplets(t, m.dim, m.c1 - m.c0, m.c0);
}

// MatrixDiagonalScale (PSMatrixAlgebraModule.F90:507-532, ScaleDiagonal.f90, sparse_includes/DiagonalScale.f90):
// for every triplet whose column is stored here, the values of that column are multiplied by its value
void ps_diagonal_scale(PSMatrix& m, const HostTriplets& t) {
  CommScope cs(m.grid);
  const int32_t width = m.c1 - m.c0;
  if (width == 0) return;
  const size_t w = m.cplx ? 2 : 1;
  std::vector<double> f((size_t)width * w, 0.0);
  for (int32_t j = 0; j < width; ++j) f[(size_t)j * w] = 1.0;
  for (size_t i = 0; i < t.size(); ++i) {
    const int32_t col = t.col[i] - 1;
    if (col < m.c0 || col >= m.c1) continue;
    double re, im = 0.0;
    if (t.cplx) { re = t.val[2 * i]; im = t.val[2 * i + 1]; } else { re = t.val[i]; }
    // several triplets naming the same column multiply one after the other, as the reference loop does
    double& fr = f[(size_t)(col - m.c0) * w];
    if (m.cplx) {
      double& fi = f[(size_t)(col - m.c0) * w + 1];
      const double nr = fr * re - fi * im, ni = fr * im + fi * re;
      fr = nr; fi = ni;
    } else {
      fr *= re;
    }
  }
  DevBuf<double> d(f.size());
  d.upload(f.data(), f.size());
  scale_columns(m.loc, d.p);
  sync_stream();  // f / d go out of scope
}

// GetMatrixBlock (PSMatrixModule.F90:1036-1150, distributed_includes/GetMatrixBlock.f90): every rank names a block
// [start_row, end_row) x [start_column, end_column) (1-based) and receives its entries with absolute coordinates;
// an entry goes to the FIRST rank whose block contains it (the EXIT in the reference's routing loop)
void ps_get_block(const PSMatrix& m, int sr, int er, int sc, int ec, HostTriplets& out) {
  CommScope cs(m.grid);
  const int P = world().active() ? world().nranks : 1, me = world().active() ? world().rank : 0;
  std::vector<int64_t> box((size_t)4 * P);
  const int64_t mine[4] = {sr, er, sc, ec};
  comm_allgather_i64(mine, 4, box.data());
  DevMat full = ps_gather_full(m);
  HostTriplets all;
  to_triplets(full, 0, all);
  out = HostTriplets();
  out.cplx = m.cplx;
  const size_t w = m.cplx ? 2 : 1;
  for (size_t i = 0; i < all.size(); ++i) {
    const int r = all.row[i], c = all.col[i];
    for (int p = 0; p < P; ++p) {
      if (r >= box[(size_t)4 * p] && r < box[(size_t)4 * p + 1] && c >= box[(size_t)4 * p + 2] && c < box[(size_t)4 * p + 3]) {
        if (p == me) {
          out.col.push_back(c);
          out.row.push_back(r);
          for (size_t k = 0; k < w; ++k) out.val.push_back(all.val[i * w + k]);
        }
        break;
      }
    }
  }
}

// GetMatrixSlice (PSMatrixModule.F90:1153-1225, distributed_includes/SliceMatrix.f90): inclusive bounds, result of
// dimension max(rows, columns) of the slice on the same grid
void ps_get_slice(const PSMatrix& m, PSMatrix& sub, int sr, int er, int sc, int ec) {
  CommScope cs(m.grid);
  HostTriplets t, s;
  ps_get_triplets(m, t);
  s.cplx = m.cplx;
  const size_t w = m.cplx ? 2 : 1;
  for (size_t i = 0; i < t.size(); ++i) {
    if (t.row[i] >= sr && t.row[i] <= er && t.col[i] >= sc && t.col[i] <= ec) {
      s.row.push_back(t.row[i] - sr + 1);
      s.col.push_back(t.col[i] - sc + 1);
      for (size_t k = 0; k < w; ++k) s.val.push_back(t.val[i * w + k]);
    }
  }
  const int new_dim = std::max(er - sr + 1, ec - sc + 1);
  const ProcessGrid* g = m.grid;
  const bool cplx = m.cplx;
  ps_construct_empty(sub, new_dim, g, cplx);
  ps_fill_from_triplets(sub, s);
}

// ResizeMatrix (PSMatrixModule.F90:1704-1741, distributed_includes/ResizeMatrix.f90): entries beyond the new size
// are dropped
void ps_resize(PSMatrix& m, int new_size) {
  CommScope cs(m.grid);
  HostTriplets t, s;
  ps_get_triplets(m, t);
  s.cplx = m.cplx;
  const size_t w = m.cplx ? 2 : 1;
  for (size_t i = 0; i < t.size(); ++i) {
    if (t.row[i] <= new_size && t.col[i] <= new_size) {
      s.row.push_back(t.row[i]);
      s.col.push_back(t.col[i]);
      for (size_t k = 0; k < w; ++k) s.val.push_back(t.val[i * w + k]);
    }
  }
  const ProcessGrid* g = m.grid;
  const bool cplx = m.cplx;
  ps_construct_empty(m, new_size, g, cplx);
  ps_fill_from_triplets(m, s);
}

int64_t ps_size(const PSMatrix& m) {
  CommScope cs(m.grid);  // GetMatrixSize (PSMatrixModule.F90:1360-1389)
  int64_t n = m.loc.nnz;
  comm_allreduce_sum_i64(&n, 1);
  return n;
}

void ps_to_complex(const PSMatrix& a, PSMatrix& out) {
  CommScope cs(a.grid);
  install(out, a.grid, a.dim, true, a.c0, a.c1, to_complex(a.loc));
}
void ps_to_real(const PSMatrix& a, PSMatrix& out) {
  CommScope cs(a.grid);
  install(out, a.grid, a.dim, false, a.c0, a.c1, to_real(a.loc));
}

// ------------------------------------------------------------------ algebra
// MatrixMultiply_ps (PSMatrixAlgebraModule.F90:108-211).  Column j of C needs column j of B
// (local) and the columns of A named by B's row indices: rank r gathers the panels of A
// (M1-M3) and multiplies them with its own panel of B; C comes out in the same panel layout, so
// there is no reduction step (slices == 1 semantics: working_threshold = threshold,
// distributed_algebra_includes/MatrixMultiply.f90:25-29).
namespace {
long long g_block_scope_products = 0;   // panel products of block-order solves (band_scope.cpp) that took the block path
long long g_panel_products[3] = {0, 0, 0};   // products of slab sessions across ranks: done in slab form on every rank; declined; host synchronisations inside the former

int panel_pitch(int32_t dim, int P, bool with_counts, int* wcols_out) {
  int32_t maxw = 0;
  for (int q = 0; q < P; ++q) {
    int32_t a0, a1;
    panel_range(dim, P, q, &a0, &a1);
    maxw = std::max(maxw, a1 - a0);
  }
  // ONE all-gather per step: every rank contributes a record of `pitch` 8-byte words -- its request (4 words), the
  // packed extents of its columns, the prefix sums of their spans and, for the statistics (timers on), their entry
  // counts; the kernels below read the sections through the common stride
  *wcols_out = maxw + 1;
  return 4 + (with_counts ? 3 : 2) * (maxw + 1);
}
// the all-gather of a step's record by a rank that has nothing to say: the others discard what they gather (collective)
void owed_allgather(int32_t dim) {
  const int P = world().nranks;
  int wcols = 0;
  const int pitch = panel_pitch(dim, P, options().time_kernels != 0, &wcols);
  DevBuf<int64_t> dummy((size_t)P * pitch);
  dummy.zero();
  world().tr->allgather(dummy.p + (size_t)world().rank * pitch, dummy.p, (size_t)pitch * sizeof(int64_t));
  sync_stream();
}
bool exchange_fits_fetch(int P) { return (size_t)4 * P + (size_t)P * P + 2 * P <= 400; }

// The exchange of the left operand's halo as dense column runs, for a panel product (panel_slab_multiply) and for a panel step
// (slab_exchange_and_step).  What it must know before the halo can travel -- every rank's request, the column extents of the
// whole left operand, who sends how much to whom, the kernel's plan -- is a function of column extents alone.  It is PREPARED
// on the device (one all-gather, three small kernels) and read back in one round trip: at the start of a product or a step,
// or -- for every step after the first -- by the step BEFORE it, from its result's extents, on that step's own read-back
// (SlabHalo::before_fetch): a panel step then costs ONE host round trip, as a step on one rank does.  Then: exchange() (layout,
// packing, one send / recv group), halo() (the layout of the columns this rank multiplies with).  The buffers live as long as
// the object: until the caller's kernel has returned (the allocator is stream ordered, and the kernels end with a read-back).
struct PanelExchange {
  int P = 0, me = 0, pitch = 0, wcols = 0, snb = 0;
  int32_t dim = 0;
  bool with_counts = false;
  bool step = false;      // a step's record (its bound is read back), not a product's
  bool planned = false;   // this rank's panel is in slab form: its plan was made
  DevBuf<int64_t> d_all, d_req, d_bound, d_cnt, plan_stats;
  SlabPlan plan;
  DevBuf<int32_t> gfirst, glast;
  std::vector<int64_t> req, bound, cnt;
  unsigned long long plan_hs[2] = {0, 0};
  const void* owner = nullptr;   // the value buffer of the iterate (in slab form) it was prepared for ...
  unsigned long long owner_serial = 0;   // ... and that buffer's allocation serial: an address alone comes back from the caching allocator
  // exchange(): the rows this rank's request names; what it sends (its columns [sa, sb) inside every requester's range, packed
  // from soff) and what it receives (the segments [ra, rb) of the other owners tile [kmin, kmax] in rank order, at zoff)
  int32_t kmin = 0, kmax = -1;
  std::vector<int32_t> sa, sb, ra, rb;
  std::vector<int64_t> soff, zoff;
  DevBuf<double> sendbuf, recvbuf;
  // halo(): the layout of the columns kmin .. kmax
  DevBuf<int32_t> d_ra, nfirst, nlast, ncount;
  DevBuf<int64_t> d_zoff;
  DevBuf<unsigned long long> naddr;
  const int64_t* d_ext_all() const { return d_all.p + 4; }
  const int64_t* d_pre_all() const { return d_all.p + 4 + wcols; }
  const int64_t* d_cnt_all() const { return with_counts ? d_all.p + 4 + 2 * (size_t)wcols : nullptr; }

  // enqueues the preparation (collective).  A step (left == nullptr): request, extents and counts of the iterate `right` in one
  // pass (d_nnz: its entry count is still on the device).  A product: the request from the rows of `right`, the extents of
  // `left`, word 3 = entries of left * 4096 + the alignment of its runs; !can: this rank's panels are not in slab form
  // (entries -1).  cplx: plan blocks of SLAB_CJ = 8 columns instead of SLAB_J = 16.
  void prepare(const DevMat& right, const DevMat* left, bool cplx, bool can, int32_t dim_, const long long* d_nnz) {
    Comm& c = world();
    P = c.nranks;
    me = c.rank;
    dim = dim_;
    step = left == nullptr;
    planned = can;
    with_counts = step && options().time_kernels != 0;
    pitch = panel_pitch(dim, P, with_counts, &wcols);
    snb = cplx ? (right.cols + 7) / 8 : (right.cols + 15) / 16;
    req.assign((size_t)4 * P, 0);
    bound.assign((size_t)2 * P, 0);
    cnt.assign((size_t)P * P, 0);
    d_all.alloc((size_t)P * pitch);
    d_req.alloc((size_t)4 * P);
    d_bound.alloc((size_t)2 * P);
    d_cnt.alloc((size_t)P * P);
    int64_t* mine = d_all.p + (size_t)me * pitch;
    if (step) {
      slab_export_async(right, mine, d_nnz, mine + 4, mine + 4 + wcols, with_counts ? mine + 4 + 2 * (size_t)wcols : nullptr);
    } else if (can) {
      slab_request_async(right, mine);
      slab_extents_async(*left, mine + 4, mine + 4 + wcols);
      const long long w3 = (long long)left->nnz * 4096 + left->slab->row_pad;
      HIP_CHECK(hipMemcpyAsync(mine + 3, &w3, sizeof(w3), hipMemcpyHostToDevice, stream()));
    } else {
      const long long rec[4] = {INT_MAX, -1, -1, 0};
      HIP_CHECK(hipMemsetAsync(mine, 0, (size_t)pitch * sizeof(int64_t), stream()));
      HIP_CHECK(hipMemcpyAsync(mine, rec, sizeof(rec), hipMemcpyHostToDevice, stream()));
    }
    c.tr->allgather(mine, d_all.p, (size_t)pitch * sizeof(int64_t));
    HIP_CHECK(hipMemcpy2DAsync(d_req.p, 4 * sizeof(int64_t), d_all.p, (size_t)pitch * sizeof(int64_t), 4 * sizeof(int64_t), (size_t)P,
                               hipMemcpyDeviceToDevice, stream()));
    halo_counts_async(d_req.p, d_pre_all(), pitch, dim, P, me, d_cnt.p, d_bound.p);   // (counts in doubles)
    // the kernel's plan (block windows and k ranges follow from the extents alone) is made here, from the gathered extents of
    // the left operand and the extents of this rank's right panel, so that its sizes come back in the same read-back as the
    // exchange layout -- a product then needs ONE more host round trip (its entry count), as on one rank
    plan_stats.alloc(24);
    if (can) {
      plan_stats.zero();
      slab_plan_panel_async(right, d_ext_all(), pitch, dim, P, plan, gfirst, glast, reinterpret_cast<unsigned long long*>(plan_stats.p));
    }
    if (step) {
      owner = right.slab->val.p;
      owner_serial = dev_alloc_serial(right.slab->val.p);
    }
  }
  // what the host needs of the preparation, on a read-back of the caller's
  void add_to(ScalarFetch& f) {
    f.add(d_req.p, 4 * P, req.data());
    if (step) f.add(d_bound.p, 2 * P, bound.data());
    f.add(d_cnt.p, P * P, cnt.data());
    if (planned) {
      f.add(plan.blk_toff.p + snb, 1, &plan.total);
      f.add(plan_stats.p + 16, 2, plan_hs);
    }
  }
  // ... or on one of its own
  void fetch() {
    if (exchange_fits_fetch(P)) {
      ScalarFetch f;
      add_to(f);
      f.run();
      return;
    }
    // (too many ranks for one fetch: plain copies)
    HIP_CHECK(hipMemcpyAsync(req.data(), d_req.p, (size_t)4 * P * 8, hipMemcpyDeviceToHost, stream()));
    if (step) HIP_CHECK(hipMemcpyAsync(bound.data(), d_bound.p, (size_t)2 * P * 8, hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)P * P * 8, hipMemcpyDeviceToHost, stream()));
    if (planned) {
      HIP_CHECK(hipMemcpyAsync(&plan.total, plan.blk_toff.p + snb, 8, hipMemcpyDeviceToHost, stream()));
      HIP_CHECK(hipMemcpyAsync(plan_hs, plan_stats.p + 16, 16, hipMemcpyDeviceToHost, stream()));
    }
    sync_stream();
  }
  // the preparation is back: the runs of the requested columns of `left` (this rank's panel of the left operand, first column
  // c0) packed per requester, one send / recv group (collective)
  void exchange(const DevMat& left, int32_t c0) {
    plan.max_w = (int)plan_hs[0];
    plan.max_kn = (int)plan_hs[1];
    kmin = req_kmin(req.data(), me);
    kmax = req_kmax(req.data(), me);
    // panel_exchange_layout: host arithmetic on the gathered requests and counts
    sa.resize((size_t)P); sb.resize((size_t)P); ra.resize((size_t)P); rb.resize((size_t)P);
    soff.assign((size_t)P + 1, 0);
    zoff.assign((size_t)P + 1, 0);
    panel_exchange_layout(dim, P, me, req.data(), cnt.data(), sa.data(), sb.data(), soff.data(), ra.data(), rb.data(), zoff.data());
    sendbuf.alloc((size_t)soff[(size_t)P] + 1);
    for (int q = 0; q < P; ++q)
      if (q != me && cnt[(size_t)me * P + q] > 0)
        slab_pack_runs_async(left, d_pre_all() + (size_t)me * pitch, sa[(size_t)q] - c0, sb[(size_t)q] - c0, sendbuf.p + soff[(size_t)q]);
    recvbuf.alloc((size_t)zoff[(size_t)P] + kIndexSlack);
    Transport& tr = *world().tr;
    tr.group_begin();
    for (int q = 0; q < P; ++q) {
      const int64_t m = cnt[(size_t)me * P + q];
      if (q != me && m > 0) tr.send(sendbuf.p + soff[(size_t)q], (size_t)m * sizeof(double), q);
    }
    for (int s = 0; s < P; ++s) {
      const int64_t m = cnt[(size_t)s * P + me];
      if (s != me && m > 0) tr.recv(recvbuf.p + zoff[(size_t)s], (size_t)m * sizeof(double), s);
    }
    tr.group_end();
  }
  // layout of the columns kmin .. kmax this rank multiplies with (kmax >= kmin): extents and run addresses, in `left` or in the
  // receive buffer, whose runs sit in slots aligned to row_pad rows
  SlabHalo halo(const DevMat& left, int row_pad) {
    const int32_t ka = kmin, kb = kmax + 1;
    d_ra.alloc((size_t)P); nfirst.alloc((size_t)(kb - ka)); nlast.alloc((size_t)(kb - ka));
    d_zoff.alloc((size_t)P);
    naddr.alloc((size_t)(kb - ka));
    if (P > 16) {   // (up to 16 ranks the segments travel as kernel arguments)
      d_ra.upload(ra.data(), (size_t)P);
      d_zoff.upload(zoff.data(), (size_t)P);
    }
    if (d_cnt_all()) ncount.alloc((size_t)(kb - ka));
    slab_halo_layout_async(d_ext_all(), d_pre_all(), pitch, dim, P, me, ka, kb, d_ra.p, d_zoff.p, recvbuf.p, left, nfirst.p, nlast.p, naddr.p,
                           d_cnt_all(), ncount.p, ra.data(), zoff.data());
    SlabHalo h;
    h.ka = ka;
    h.kb = kb;
    h.first = nfirst.p;
    h.last = nlast.p;
    h.addr = naddr.p;
    h.count = ncount.p;
    h.row_pad = row_pad;
    h.plan = &plan;
    return h;
  }
};
std::unique_ptr<PanelExchange> g_pending_exchange;
long long g_exchange_prefetched = 0;   // panel steps whose exchange layout came with the step before
}  // namespace
// the preparation a step left for a successor that never came (the last step of a solve or of a bench block): P * pitch * 8
// bytes of device memory and a stale layout -- dropped where a solve begins and ends and with the operand caches
void drop_pending_exchange() { g_pending_exchange.reset(); }
namespace {

// C = alpha A B of a slab session on more than one rank: A, B column panels in slab form, the result a column panel in slab
// form (MatrixMultiply.f90:92-267 gathers blocks of both operands along the grid; here the rows of B's panel name the columns
// of A that have to travel, as dense runs).  Protocol, all on the engine stream: (1) ONE all-gather of a record per rank --
// request (first / last row of B's panel, entries of B, entries of A and the alignment of its runs; -1: this rank's panels are
// not in slab form), packed extents of A's columns, prefix sums of their spans; (2) who sends how many doubles to whom, one
// read-back (PanelExchange prepare, fetch); (3) the runs of the requested columns packed per requester, one send / recv group
// (exchange); (4) layout of the columns this rank multiplies with (halo), the tile kernel on them (slab_multiply with a left
// halo); (5) one reduction: did every rank's kernel take its panel.  Collective; false (every rank alike): nothing done, the
// caller takes the compressed-column path.
bool panel_slab_multiply(const PSMatrix& A, const PSMatrix& B, DevMat& AB, double alpha, double threshold) {
  Transport& tr = *world().tr;
  const int P = world().nranks;
  const long long syncs_before = host_sync_count();
  // (complex operands, a session that takes them: runs of (re, im) pairs -- twice the doubles per row in the exchange, a plan of
  // SLAB_CJ columns per block, the complex tile kernel)
  const SlabKind& k = slab_kind(A.cplx);
  const bool mine_ok = slab_on() && A.loc.nnz > 0 && B.loc.nnz > 0 && A.c0 == B.c0 && A.c1 == B.c1 && k.enter(mut(A)) &&
                       (&A == &B || k.enter(mut(B))) && A.loc.slab->row_pad % 16 == 0 && A.loc.slab->row_pad < 4096;
  PanelExchange pe;
  pe.prepare(B.loc, &A.loc, A.cplx, mine_ok, A.dim, nullptr);
  pe.fetch();
  exchange_stats().exchanges += 1;
  const std::vector<int64_t>& req = pe.req;
  int64_t nnz_a = 0, nnz_b = 0;
  bool all_ok = true;
  for (int q = 0; q < P; ++q) {
    if (req[(size_t)4 * q + 2] < 0) { all_ok = false; break; }
    nnz_b += req[(size_t)4 * q + 2];
    nnz_a += req[(size_t)4 * q + 3] / 4096;
    if (req[(size_t)4 * q + 3] % 4096 != req[3] % 4096) all_ok = false;   // (every panel's runs aligned alike)
  }
  if (!all_ok) {
    g_panel_products[1] += 1;
    return false;
  }
  const int row_pad = (int)(req[3] % 4096);
  pe.exchange(A.loc, A.c0);
  // "did every rank's kernel take its panel": known to a rank once its plan is back; the sum over the ranks is enqueued
  // here and read back with the product's entry count
  // (the SAME predicate slab_multiply applies -- a rank that agrees here cannot decline later)
  const bool ok = mine_ok && pe.kmax >= pe.kmin && k.takes_panel(A.loc, B.loc, row_pad, pe.kmin, pe.kmax + 1, &pe.plan);
  DevBuf<double> d_declined(4);
  double declined[4] = {ok ? 0.0 : 1.0, 0.0, 0.0, 0.0};
  d_declined.upload(declined, 4);
  tr.allreduce(d_declined.p, 4, true, 0);
  bool fetched = false;
  if (ok) {
    SlabHalo halo = pe.halo(A.loc, row_pad);
    // (a thin operand: the gather kernels, decided on the entry counts of the whole operands -- they came with the requests --
    // and the global dimension: the same on every rank, and what one rank decides for this product)
    halo.thin = slab_thin_rule(nnz_a, nnz_b, A.dim);
    halo.nnz_a = nnz_a;
    halo.on_fetch = [&](ScalarFetch& f) {
      f.add(d_declined.p, 1, reinterpret_cast<unsigned long long*>(&declined[0]));
      fetched = true;
    };
    if (!k.multiply(A.loc, B.loc, AB, alpha, threshold, dense_branch(A.dim, nnz_a, nnz_b), &halo))
      NTP_FATAL("internal: a panel product was declined after its rank had agreed to it");
  }
  if (!fetched) {
    ScalarFetch f;
    f.add(d_declined.p, 1, reinterpret_cast<unsigned long long*>(&declined[0]));
    f.run();
  }
  if (declined[0] != 0.0) {
    g_panel_products[1] += 1;
    return false;
  }
  g_panel_products[0] += 1;
  g_panel_products[2] += host_sync_count() - syncs_before;   // (measured in sync_stream: the exchange's and the product's)
  return true;
}
}  // namespace
const long long* panel_product_counts() { return g_panel_products; }
long long block_scope_products() { return g_block_scope_products; }

namespace {
// alpha * A * B with the threshold, local panel of the result (slices == 1 semantics: every output entry is one sum
// over the whole inner dimension in ascending order)
DevMat multiply_panel(const PSMatrix& A, const PSMatrix& B, double alpha, double threshold, double a_fraction = 1.0) {
  // dense-branch rule of the local multiply (GemmMatrix.f90:49-61): only the order of threshold and
  // alpha differs here, the arithmetic is the same hash-free sparse kernel.  a_fraction: share of the inner dimension
  // A is populated over (a process slice's operand: its density is that of the populated part, as in the
  // reference's per-block test)
  int64_t nz[2] = {A.loc.nnz, B.loc.nnz};
  DevMat AB;
  if (world().active()) {
    // only the columns of A named by the rows of the local B panel travel (halo for banded operands); the same
    // exchange returns the global nnz for the dense-branch rule
    HaloExchange hx;
    gather_needed_begin(hx, A, B.loc, nz, true);
    const bool dense_rule = dense_branch(A.dim, nz[0], nz[1], a_fraction);
    const ColRange need{hx.kmin, hx.kmax + 1};   // the rows of the B panel name these columns only
    // A solve in a block order (band_scope.cpp: 3-D operands on several ranks): the panel of B as the columns c0 .. c1 of a
    // square matrix whose other columns are empty, the product through the block path -- tiles of the order the scope
    // installed, candidates in this rank's super-columns only -- and the panel's columns cut out of the result.  Complex
    // operands (a complex first operand's scope, option block_scope_complex) the same way, on the complex tile products of the
    // block path (k_bs_numeric_c); a real operand beside a complex one arrives here up-cast (ps_multiply), as on one rank.  The
    // route depends only on what every rank sees alike -- the options, the operands' kinds, the scope -- so no rank declines it
    // alone (the block path's own refusal is local: that rank's product then goes to the LDS hash, no collective follows)
    const bool kinds_ok = A.cplx == B.cplx && (!A.cplx || (options().block_scope_complex != 0 && complex_forms_ok()));
    const bool block_route = block_scope_active() && kinds_ok && options().spgemm_fma == 1 && options().block_path != 0 && a_fraction == 1.0;
    if (block_route) {
      hx.finish();
      DevMat Csq;
      {
        MatView Bsq;
        DevBuf<int64_t> pad_outer((size_t)B.dim + 1);
        fill_i64(pad_outer.p, B.c0, 0);
        copy_shift_i64(B.loc.outer.p, pad_outer.p + B.c0, (int64_t)(B.c1 - B.c0) + 1, 0);
        fill_i64(pad_outer.p + B.c1 + 1, (int64_t)B.dim - B.c1, B.loc.nnz);
        Bsq.alias(B.loc, pad_outer.p, B.dim, B.loc.nnz);
        hx.full.block_hint = 1;   // (straight to the block path: no run statistics, no band search on the gathered operand)
        // (complex: no fill floor -- an iterate that has thinned out, 3 I - X^2 late in a sign loop at fill 0.075, would otherwise
        // send the whole gathered operand to the general kernels: minutes for one product of a 40^3 lattice, against 0.1 s here)
        BlockForceScope force(A.cplx);
        spgemm(hx.full, Bsq.m, Csq, alpha, threshold, dense_rule);
        sync_stream();   // (the padded offsets are released on leaving the scope)
      }
      if (last_spgemm_stats().block) g_block_scope_products += 1;
      if (Csq.loose() || Csq.expanded() || Csq.blocked()) pack(Csq);
      MatView Cv;
      Cv.alias(Csq, Csq.outer.p + B.c0, B.c1 - B.c0, Csq.nnz);
      AB = concat_columns({&Cv.m});
      sync_stream();
    } else if (!hx.overlapped) {
      hx.finish();
      spgemm(hx.full, B.loc, AB, alpha, threshold, dense_rule, nullptr, &need);
    } else {
      // the halo is travelling on the communication stream: multiply the interior columns of the B panel (they
      // name local columns of A only) meanwhile, then the boundary columns against the gathered operand.  A
      // column's arithmetic does not depend on which call computes it, so the result is bit-identical.
      const int32_t width = B.c1 - B.c0;
      DevMat Cint, Cleft, Cright;
      {
        MatView Apad, Bint;
        DevBuf<int64_t> pad_outer((size_t)A.dim + 1);
        fill_i64(pad_outer.p, A.c0, 0);
        copy_shift_i64(A.loc.outer.p, pad_outer.p + A.c0, (int64_t)(A.c1 - A.c0) + 1, 0);
        fill_i64(pad_outer.p + A.c1 + 1, (int64_t)A.dim - A.c1, A.loc.nnz);
        Apad.alias(A.loc, pad_outer.p, A.dim, A.loc.nnz);
        Bint.alias(B.loc, B.loc.outer.p + hx.jl, hx.jr - hx.jl, hx.off_r - hx.off_l);
        spgemm(Apad.m, Bint.m, Cint, alpha, threshold, dense_rule);
      }
      hx.finish();
      if (hx.jl > 0) {
        MatView Bl;
        Bl.alias(B.loc, B.loc.outer.p, hx.jl, hx.off_l);
        spgemm(hx.full, Bl.m, Cleft, alpha, threshold, dense_rule, nullptr, &need);
      } else {
        Cleft.reset_empty(A.dim, 0, A.cplx);
      }
      if (hx.jr < width) {
        MatView Br;
        Br.alias(B.loc, B.loc.outer.p + hx.jr, width - hx.jr, B.loc.nnz - hx.off_r);
        spgemm(hx.full, Br.m, Cright, alpha, threshold, dense_rule, nullptr, &need);
      } else {
        Cright.reset_empty(A.dim, 0, A.cplx);
      }
      std::vector<const DevMat*> parts;
      if (Cleft.cols) parts.push_back(&Cleft);
      parts.push_back(&Cint);
      if (Cright.cols) parts.push_back(&Cright);
      AB = parts.size() == 1 ? std::move(Cint) : concat_columns(parts);
    }
  } else {
    spgemm(A.loc, B.loc, AB, alpha, threshold, dense_branch(A.dim, nz[0], nz[1], a_fraction));
  }
  return AB;
}
}  // namespace

void ps_multiply(const PSMatrix& A, const PSMatrix& B, PSMatrix& C, double alpha, double beta, double threshold) {
  CommScope cs(A.grid);
  if (A.dim != B.dim) NTP_FATAL("MatrixMultiply: dimension mismatch");
  // up-casting of mixed real/complex operands (PSMatrixAlgebraModule.F90:171-188)
  if (A.cplx != B.cplx) {
    // (a real operand that an earlier call of a slab session left in slab form or loose: to_complex copies the three
    // arrays of compressed columns, so the operands are packed first)
    if (A.loc.expanded() || A.loc.loose() || A.loc.blocked()) pack(mut(A));
    if (B.loc.expanded() || B.loc.loose() || B.loc.blocked()) pack(mut(B));
    PSMatrix Ac, Bc;
    ps_to_complex(A, Ac);
    ps_to_complex(B, Bc);
    ps_multiply(Ac, Bc, C, alpha, beta, threshold);
    return;
  }
  DevMat AB;
  const int S = A.grid ? A.grid->num_slices : 1;
  // A one-call session of the C ABI on operands without run structure (or already in block form): the product goes
  // through the block path and STAYS in block form (DevMat::blk) -- the next product of the caller's loop multiplies it
  // as it is, every other entry point packs on access.  Solver loops (sessions of their own) take compressed columns.
  // Complex operands the same way where complex block forms are allowed (complex_blocks_on) -- before a complex session's
  // attempt on runs, whose refusals would end the session
  const bool block_first = slab_on() && (!A.cplx || complex_blocks_on()) && S <= 1 && beta_is_zero(beta) &&
                           (A.loc.blocked() || B.loc.blocked() || A.loc.block_hint || B.loc.block_hint) && !A.loc.expanded() && !B.loc.expanded() &&
                           !A.loc.loose() && !B.loc.loose();
  if (block_first) {
    BlockKeepScope keep;
    spgemm(A.loc, B.loc, AB, alpha, threshold, dense_branch(A.dim, A.loc.nnz, B.loc.nnz));
    install(C, A.grid, A.dim, A.cplx, B.c0, B.c1, std::move(AB));
    return;
  }
  unblock({&A, &B});
  // (real operands, or complex ones in a session that takes them)
  const bool in_slab_form = session_takes(A.cplx) && S <= 1 && beta_is_zero(beta);
  const SlabKind& k = slab_kind(A.cplx);
  if (g_slab_depth > 0 && world().active() && in_slab_form) {
    // (a slab session across ranks: collective -- every rank reports whether its panels are in slab form with the halo request,
    // and every rank takes the same branch)
    if (panel_slab_multiply(A, B, AB, alpha, threshold)) {
      g_slab_counts[0] += 1;
      count_view_product(A, B);
      install(C, A.grid, A.dim, A.cplx, B.c0, B.c1, std::move(AB));
      return;
    }
    g_slab_counts[3] += 1;
    for (const PSMatrix* m : {&A, &B})
      if (m->loc.expanded() || m->loc.loose()) pack(mut(*m));
  } else if (slab_on() && !world().active() && in_slab_form && A.loc.nnz > 0 && B.loc.nnz > 0) {
    // (a slab session: operands are turned into slab form where they are, the product stays in it -- complex iterates in the
    // complex tile kernel's operand form)
    // (unfused arithmetic, real: the register-slab kernel multiplies whole runs, zeros included -- operands that have become
    // sparse inside wide extents, 3 I - X^2 near the end of a sign iteration, are better served by the general kernels,
    // which the compressed-column path picks per product; the MFMA tile kernel of the FMA mode takes them as they are)
    // (the Polar session keeps them all the same, slab_keep_sparse_runs: a product handed over packs the iterate, and the next
    // transpose and product would start from compressed columns again)
    auto runs_dense = [](const DevMat& M) {
      return options().spgemm_fma != 0 || g_keep_sparse_runs || !M.expanded() || (double)slab_span_sum(M) <= 1.5 * (double)M.nnz + 64.0 * (double)M.cols;
    };
    if (k.enter(mut(A)) && (&A == &B || k.enter(mut(B))) && (A.cplx || (runs_dense(A.loc) && runs_dense(B.loc))) &&
        k.multiply(A.loc, B.loc, AB, alpha, threshold, dense_branch(A.dim, A.loc.nnz, B.loc.nnz), nullptr)) {
      g_slab_counts[0] += 1;
      count_view_product(A, B);
      if (!A.cplx && options().time_kernels != 0) {   // (statistics mode: the products a plan over compressed columns would have counted)
        const long long pr = slab_product_count(A.loc, B.loc);
        last_spgemm_stats().products = pr;
        spgemm_accum().products += pr;
      }
      install(C, A.grid, A.dim, A.cplx, B.c0, B.c1, std::move(AB));
      return;
    }
    slab_refused({&A, &B});
  } else {
    slab_pack_if({&A, &B});
  }
  if ((C.loc.expanded() || C.loc.loose() || C.loc.blocked()) && &C != &A && &C != &B) pack(C.loc);   // (beta != 0 reads it below; otherwise it is replaced)
  if (S <= 1) {
    // (a one-call session of the C ABI: should the product turn out to belong to the block path -- decided inside spgemm()
    // once the run-based kernels have declined -- it stays in block form, and the refusal above was not one)
    std::optional<BlockKeepScope> keep;
    if (g_slab_depth > 0 && !g_slab_failed && (!A.cplx || complex_blocks_on()) && beta_is_zero(beta)) keep.emplace();
    AB = multiply_panel(A, B, alpha, threshold);
    keep.reset();
    if (AB.blocked() && g_slab_refusals > 0) { g_slab_refusals -= 1; }
  } else {
    // Process slices (the reference's 2.5-D algorithm, MatrixMultiply.f90:25-29, 74-80, 230-267): slice s multiplies
    // its share of the inner dimension -- the blocks g with g % S == s, block = padded dimension / (max(rows, columns)
    // * S * block multiplier) -- with threshold / (1000 S); the partial products are then summed in slice order by
    // IncrementMatrix, only the last addition with the caller's threshold (comm_includes/ReduceAndSumMatrixCleanup.f90
    // :11-32), so entries below the threshold survive where the rule copies tails unfiltered.  This engine keeps its
    // column panels and reproduces those sums: S multiplies over masked copies of A, S increments.  (Block multiplier 1
    // = the reference run with fewer threads than blocks.)
    const ProcessGrid& g = *A.grid;
    const int64_t lcm = (int64_t)S * g.num_cols * g.num_rows;
    const int64_t padded = ((int64_t)A.dim + lcm - 1) / lcm * lcm;
    const int32_t block = (int32_t)(padded / ((int64_t)std::max(g.num_rows, g.num_cols) * S));
    const double working = threshold / ((double)S * 1000.0);
    AB.reset_empty(A.dim, B.c1 - B.c0, A.cplx);
    for (int s = 0; s < S; ++s) {
      PSMatrix As;
      install(As, A.grid, A.dim, A.cplx, A.c0, A.c1, mask_columns(A.loc, A.c0, block, S, s));
      int64_t kcount = 0;   // columns of the whole matrix in this slice's share
      for (int64_t k0 = (int64_t)s * block; k0 < A.dim; k0 += (int64_t)S * block) kcount += std::min<int64_t>(block, A.dim - k0);
      DevMat part = multiply_panel(As, B, alpha, working, std::max(1e-300, (double)kcount / (double)A.dim));
      increment_blocked(part, AB, 1.0, s == S - 1 ? threshold : 0.0, block);   // (row blocks = inner-dimension blocks)
    }
  }
  // beta handling (MatrixMultiply.f90:324-329)
  if (beta_is_zero(beta) || !C.constructed() || C.dim != A.dim) {
    install(C, A.grid, A.dim, A.cplx, B.c0, B.c1, std::move(AB));
  } else {
    if (C.cplx != A.cplx) {
      PSMatrix Cc;
      ps_to_complex(C, Cc);
      C.cplx = true;
      C.loc = std::move(Cc.loc);
      if (!A.cplx) AB = to_complex(AB);
    }
    scale(C.loc, beta);
    increment(AB, C.loc, 1.0, 0.0);
  }
}

// IncrementMatrix_ps (PSMatrixAlgebraModule.F90:414-460)
void ps_increment(const PSMatrix& A, PSMatrix& B, double alpha, double threshold) {
  CommScope cs(A.grid);
  if (A.dim != B.dim) NTP_FATAL("IncrementMatrix: dimension mismatch");
  if (blk_any({&A, &B}) && &A != &B && blk_kinds(A, B)) {
    ps_axpby(A, B, alpha, 1.0, threshold);
    return;
  }
  unblock({&A, &B});
  if (slab_on() && (A.loc.expanded() || B.loc.expanded()) && &A != &B) {
    ps_axpby(A, B, alpha, 1.0, threshold);
    return;
  }
  slab_pack_if({&A, &B});
  if (A.cplx && !B.cplx) {
    DevMat bc = to_complex(B.loc);
    increment(A.loc, bc, alpha, threshold);
    B.cplx = true;
    B.loc = std::move(bc);
  } else if (!A.cplx && B.cplx) {
    DevMat ac = to_complex(A.loc);
    increment(ac, B.loc, alpha, threshold);
  } else if (&A == &B) {
    DevMat a2 = A.loc.clone();
    increment(a2, B.loc, alpha, threshold);
  } else {
    increment(A.loc, B.loc, alpha, threshold);
  }
}

void ps_scale(PSMatrix& A, double c) {
  CommScope cs(A.grid);
  if (blk_any({&A})) {
    if (block_scale(A.loc, c)) { g_block_counts[0] += 1; return; }
    g_block_counts[1] += 1;
  }
  unblock({&A});
  if (slab_on() && A.loc.expanded()) {
    // (a complex operand outside a session that takes them is refused: the real slab_scale declines it untouched)
    if (session_takes(A.cplx) && slab_kind(A.cplx).scale(A.loc, c)) { g_slab_counts[2] += 1; return; }
    slab_refused({&A});
  }
  scale(A.loc, c);
}

// B <- alpha*A + beta*B: ScaleMatrix(B, beta) followed by IncrementMatrix(A, B, alpha, threshold) in one pass (the
// merge kernels scale B's values as they read them: the same products, the same rules, bit for bit)
void ps_axpby(const PSMatrix& A, PSMatrix& B, double alpha, double beta, double threshold) {
  CommScope cs(A.grid);
  if (A.dim != B.dim) NTP_FATAL("IncrementMatrix: dimension mismatch");
  if (blk_any({&A, &B}) && blk_kinds(A, B) && &A != &B && !A.loc.expanded() && !B.loc.expanded() && !A.loc.loose() && !B.loc.loose()) {
    if (block_axpby(A.loc, B.loc, alpha, beta, threshold)) {
      g_block_counts[0] += 1;
      B.cplx = B.loc.cplx;   // (a real B beside a complex A: up-cast, as IncrementMatrix)
      return;
    }
    g_block_counts[1] += 1;
  }
  unblock({&A, &B});
  if (slab_on() && (A.loc.expanded() || B.loc.expanded()) && A.cplx == B.cplx && session_takes(A.cplx) && &A != &B) {
    // (a slab session: the operand still in compressed columns -- an identity, the Hamiltonian -- is turned into slab form;
    // complex operands in a session that takes them: the merge on runs of (re, im) pairs; mixed kinds: the general path)
    const SlabKind& k = slab_kind(A.cplx);
    const long long declined = slab_view_counts()[3];
    if (k.enter(mut(A)) && k.enter(B.loc) && k.axpby(A.loc, B.loc, alpha, beta, threshold)) { g_slab_counts[1] += 1; return; }
    if (slab_view_counts()[3] != declined) {
      slab_refused_view_merge();
      DevMat tmp;
      const DevMat& Ac = columns_of(A, tmp);
      pack(B.loc);   // (B is replaced by the result, which stores a zero: compressed columns)
      axpby(Ac, B.loc, alpha, beta, threshold, nullptr, nullptr);
      return;
    }
    slab_refused({&A, &B});
  } else {
    slab_pack_if({&A, &B});
  }
  if (A.cplx != B.cplx || &A == &B) {
    ps_scale(B, beta);
    ps_increment(A, B, alpha, threshold);
    return;
  }
  axpby(A.loc, B.loc, alpha, beta, threshold, nullptr, nullptr);
}

void ps_increment_identity(const PSMatrix& Identity, PSMatrix& B, double alpha) {
  CommScope cs(Identity.grid);
  // (a real B takes a real identity only; never counted as a refusal: the paths below take what the slab form declines)
  if (slab_on() && B.loc.expanded() && session_takes(B.cplx) && (B.cplx || !Identity.cplx) && Identity.dim == B.dim &&
      slab_kind(B.cplx).add_diagonal(B.loc, alpha, B.c0)) {
    g_slab_counts[1] += 1;
    return;
  }
  // compressed columns that store their diagonal: one value per column changes, in place
  if (options().column_fused != 0 && Identity.dim == B.dim && (!Identity.cplx || B.cplx) && !B.loc.expanded() && !B.loc.loose() && !B.loc.blocked() &&
      add_identity_inplace(B.loc, alpha, B.c0)) {
    g_column_fused[0] += 1;
    return;
  }
  ps_increment(Identity, B, alpha, 0.0);
}

bool ps_norm_axpby(const PSMatrix& A, const PSMatrix& B, double alpha, double beta, double* norm) {
  CommScope cs(A.grid);
  if (blk_any({&A, &B})) return false;   // (the caller spells it with the vocabulary, which knows the block form)
  const bool in_slab_form = slab_on() && (A.loc.expanded() || B.loc.expanded());
  if (A.cplx == B.cplx && session_takes(A.cplx) && A.dim == B.dim && &A != &B && (world().active() ? g_slab_depth > 0 : in_slab_form)) {
    const SlabKind& k = slab_kind(A.cplx);
    double v = 0.0;
    const bool ok = in_slab_form && k.enter(mut(A)) && k.enter(mut(B)) && k.norm_axpby(A.loc, B.loc, alpha, beta, &v);
    if (world().active()) {
      // (a session across ranks: the decision is collective -- one reduction carries the norm and "some rank declined",
      // whether or not this rank could)
      double pair[2] = {ok ? v : 0.0, ok ? 0.0 : 1.0};
      comm_allreduce_max(pair, 2);
      if (pair[1] != 0.0) return false;
      v = pair[0];
    } else if (!ok) {
      return false;
    }
    *norm = v;
    g_slab_counts[2] += 1;
    return true;
  }
  // compressed columns (complex loops, real ones outside a session): a dense window per column, the difference is never formed
  auto cols = [](const PSMatrix& M) { return !M.loc.expanded() && !M.loc.loose() && !M.loc.blocked(); };
  if (options().column_fused != 0 && beta == 1.0 && A.cplx == B.cplx && A.dim == B.dim && &A != &B && cols(A) && cols(B) && A.c0 == B.c0 && A.c1 == B.c1) {
    // (the decision is collective: a rank whose columns do not fit the kernel's window must not fall back alone -- one
    // reduction carries the norm and "some rank declined" together, and every rank takes the same branch)
    double v = 0.0;
    const bool ok = norm_axpy_columns(A.loc, B.loc, alpha, &v);
    double pair[2] = {ok ? v : 0.0, ok ? 0.0 : 1.0};
    comm_allreduce_max(pair, 2);
    if (pair[1] == 0.0) {
      *norm = pair[0];
      g_column_fused[1] += 1;
      return true;
    }
  }
  return false;
}

bool ps_recurrence_step(const PSMatrix& P, const PSMatrix& Tkm2, PSMatrix& Tk, PSMatrix& R, double a, double c) {
  CommScope cs(P.grid);
  if (options().complex_poly_sessions != 2 || !slab_on() || !P.cplx || !Tkm2.cplx || !R.cplx || !session_takes(true)) return false;
  if (blk_any({&P, &Tkm2, &R}) || P.dim != Tkm2.dim || P.dim != R.dim || &P == &Tkm2 || &P == &R || &Tkm2 == &R || &Tk == &R || &Tk == &Tkm2)
    return false;
  // (an operand still in compressed columns -- the identity as T0, the input as T1, the sum before the first product -- is
  // turned into slab form as ps_axpby would; one that cannot be is left to the two merges, which count the refusal.  Every
  // rank of a panel session decides for itself: neither this step nor the two merges hold a collective)
  if (!(P.loc.expanded() || Tkm2.loc.expanded() || R.loc.expanded()) || !slab_enter_c(mut(P)) || !slab_enter_c(mut(Tkm2)) || !slab_enter_c(R.loc))
    return false;
  DevMat T;
  if (!slab_recurrence_step_c(P.loc, Tkm2.loc, T, R.loc, a, c)) return false;
  install(Tk, P.grid, P.dim, true, P.c0, P.c1, std::move(T));
  g_slab_counts[1] += 2;
  g_recurrence_steps += 1;
  return true;
}

long long* complex_trs4_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// the gates of the complex TRS4 passes (option complex_trs4): the option, one rank, an open session that takes complex operands,
// complex operands of one dimension that are not in block form.  A pass they keep out is neither fused nor counted as refused
// (option: the value of the loop's own option -- complex_trs4 here, complex_hpcp for the HPCP passes below)
bool complex_passes_on(int option, std::initializer_list<const PSMatrix*> ms) {
  if (option == 0 || world().active() || !slab_on() || !session_takes(true) || blk_any(ms)) return false;
  const PSMatrix* first = *ms.begin();
  for (const PSMatrix* m : ms)
    if (!m->cplx || m->dim != first->dim || m->loc.blocked() || m->loc.loose()) return false;
  return true;
}
bool ctrs4_on(std::initializer_list<const PSMatrix*> ms) { return complex_passes_on(options().complex_trs4, ms); }
// ... and in the loop: both merged operands in complex slab form as the products left them, neither labelled
bool ctrs4_in_slab_form(const PSMatrix& X, const PSMatrix& X2) {
  return &X != &X2 && X.loc.expanded() && X2.loc.expanded() && !labelled(X) && !labelled(X2);
}
// the loop's gates on one rank: both operands of one kind in slab form -- complex ones under ctrs4_on, real ones in any session
bool trs4_in_loop(const PSMatrix& X, const PSMatrix& X2) {
  if (X.cplx && X2.cplx) return ctrs4_on({&X, &X2}) && ctrs4_in_slab_form(X, X2);   // (option complex_trs4; one rank)
  return slab_on() && X.loc.expanded() && X2.loc.expanded() && !X.cplx && !X2.cplx;
}
// the two passes past their gates, on operands of one kind in slab form
bool trs4_traces_local(const PSMatrix& X, const PSMatrix& X2, double* trace_fx, double* trace_gx) {
  return X.cplx ? slab_trs4_traces_c(X.loc, X2.loc, X.c0, trace_fx, trace_gx) : slab_trs4_traces(X.loc, X2.loc, X.c0, trace_fx, trace_gx);
}
bool trs4_operand_local(const PSMatrix& X, const PSMatrix& X2, double sigma, DevMat& R) {
  return X.cplx ? slab_trs4_operand_c(X.loc, X2.loc, sigma, X.c0, R) : slab_trs4_operand(X.loc, X2.loc, sigma, X.c0, R);
}
// ... and their books (pass 0: the traces, 1: the operand): slab_algebra_counts() counts a fused pass of either kind,
// complex_trs4_counts() the complex ones -- and a complex pass the kernel does not take as refused.  Returns ok
bool trs4_counted(bool cplx, int pass, bool ok) {
  if (ok) {
    g_slab_counts[pass == 0 ? 2 : 1] += 1;
    if (cplx) complex_trs4_counts()[pass] += 1;
  } else if (cplx) {
    complex_trs4_counts()[3] += 1;
  }
  return ok;
}
}  // namespace

bool ps_trs4_traces(const PSMatrix& X, const PSMatrix& X2, double* trace_fx, double* trace_gx) {
  CommScope cs(X.grid);
  if (blk_any({&X, &X2})) return false;   // (the caller spells it with the vocabulary, which knows the block form)
  if (X.cplx && X2.cplx)   // (option complex_trs4; one rank)
    return trs4_in_loop(X, X2) && trs4_counted(true, 0, trs4_traces_local(X, X2, trace_fx, trace_gx));
  if (world().active()) {
    // (a session across ranks: the decision is collective -- the sums and "some rank declined" in one reduction)
    if (g_slab_depth == 0 || X.cplx || X2.cplx) return false;
    double t[3] = {0.0, 0.0, 0.0};
    const bool ok = slab_on() && X.loc.expanded() && X2.loc.expanded() && slab_trs4_traces(X.loc, X2.loc, X.c0, &t[0], &t[1]);
    if (!ok) { t[0] = t[1] = 0.0; t[2] = 1.0; }
    comm_allreduce_sum(t, 3);
    if (t[2] != 0.0) return false;
    *trace_fx = t[0];
    *trace_gx = t[1];
    g_slab_counts[2] += 1;
    return true;
  }
  return trs4_in_loop(X, X2) && trs4_counted(false, 0, trs4_traces_local(X, X2, trace_fx, trace_gx));
}
bool ps_trs4_operand(const PSMatrix& X, const PSMatrix& X2, double sigma, PSMatrix& P) {
  CommScope cs(X.grid);
  if (blk_any({&X, &X2})) return false;   // (the caller spells it with the vocabulary, which knows the block form)
  DevMat R;
  if (!trs4_in_loop(X, X2) || sigma == 0.0 || !trs4_counted(X.cplx, 1, trs4_operand_local(X, X2, sigma, R))) return false;
  install_like(P, X, X.cplx, std::move(R));
  return true;
}
bool ps_trs4_energy(const PSMatrix& X, const PSMatrix& WH, double* energy) {
  CommScope cs(X.grid);
  // (WH as it stands: complex slab form, a read-only view, or compressed columns -- stored zeros add exact zeros to the sum)
  if (&X == &WH || !ctrs4_on({&X, &WH}) || !X.loc.expanded() || labelled(X) || labelled(WH)) return false;
  double dot[2] = {0.0, 0.0};
  if (!sa_operand_c(X.loc) || !slab_dot_trace_c(X.loc, &WH.loc, X.c0, dot, nullptr)) {
    complex_trs4_counts()[3] += 1;
    return false;
  }
  *energy = dot[0];
  g_slab_counts[2] += 1;
  complex_trs4_counts()[2] += 1;
  return true;
}
bool ps_trs4_chain_step(const PSMatrix& X, const PSMatrix& X2, double sigma, PSMatrix& P, double* trace_fx, double* trace_gx) {
  CommScope cs(X.grid);
  if (world().active() || !slab_on() || X.cplx != X2.cplx || !same_dim({&X, &X2}) || !all_distinct({&X, &X2, &P}) || sigma == 0.0) return false;
  if (X.cplx && !ctrs4_on({&X, &X2})) return false;
  unblock({&X, &X2});
  if (labelled(X) || labelled(X2)) return false;
  const SlabKind& k = slab_kind(X.cplx);
  double t[2] = {0.0, 0.0};
  DevMat R;
  if (!(k.enter(mut(X)) && k.enter(mut(X2)) && trs4_traces_local(X, X2, &t[0], &t[1]) && trs4_operand_local(X, X2, sigma, R)))
    return trs4_counted(X.cplx, 0, false);   // (one refusal, whichever of them declined)
  pack(R);
  install_like(P, X, X.cplx, std::move(R));
  *trace_fx = t[0];
  *trace_gx = t[1];
  return trs4_counted(X.cplx, 0, true) && trs4_counted(X.cplx, 1, true);
}
bool ps_trs4_energy_step(const PSMatrix& X, const PSMatrix& WH, double* energy) {
  CommScope cs(X.grid);
  if (&X == &WH || !ctrs4_on({&X, &WH})) return false;
  if (!X.loc.expanded() && !slab_enter_c(mut(X), nullptr, false)) {
    complex_trs4_counts()[3] += 1;
    return false;
  }
  return ps_trs4_energy(X, WH, energy);
}

long long* isr_chain_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
namespace {
// the gates of the fused chain: the option, an open session that takes the operands' kind, an operand in slab form (in unfused
// arithmetic a product whose operands are sparse inside wide extents goes to the general kernels: an X and an X X that both come
// back in compressed columns are left to the vocabulary, which decides call by call), none of them in labelled slab form (a
// relabelled band: the kernel walks rows in the caller's order).  A step the gates keep out is neither fused nor counted as refused
bool isr_chain_on(const PSMatrix& X, const PSMatrix& X2) {
  return options().isr_chain != 0 && slab_on() && X.cplx == X2.cplx && session_takes(X.cplx) && X.dim == X2.dim && &X != &X2 &&
         !blk_any({&X, &X2}) && (X.loc.expanded() || X2.loc.expanded()) && !labelled(X) && !labelled(X2);
}
// the chain past its gates: an operand still in compressed columns is turned into slab form where it is, as ps_axpby does before
// a merge, and one chain of the given order leaves q (and p, order 5).  Counted as fused -- in slab_algebra_counts() as the merges
// replaced -- or as refused
bool isr_chain_local(const PSMatrix& X, const PSMatrix& X2, int order, double a, double b, double c, DevMat& q, DevMat& p) {
  const SlabKind& k = slab_kind(X.cplx);
  if (!(k.enter(mut(X)) && k.enter(mut(X2)) &&
        (order == 5 ? slab_isr_chain5(X.loc, X2.loc, a, b, c, X.c0, q, p) : slab_isr_chain3(X.loc, X2.loc, X.c0, q)))) {
    isr_chain_counts()[2] += 1;
    return false;
  }
  g_slab_counts[1] += order == 5 ? 4 : 2;
  isr_chain_counts()[order == 5 ? 0 : 1] += 1;
  return true;
}
}  // namespace
bool ps_isr_chain5(const PSMatrix& X, const PSMatrix& X2, double a, double b, double c, PSMatrix& Temp2, PSMatrix& Temp) {
  CommScope cs(X.grid);
  DevMat q, p;
  if (!isr_chain_on(X, X2) || !isr_chain_local(X, X2, 5, a, b, c, q, p)) return false;
  const bool cplx = X.cplx;
  install_like(Temp2, X, cplx, std::move(q));
  install_like(Temp, X, cplx, std::move(p));
  return true;
}
bool ps_isr_chain3(PSMatrix& X, const PSMatrix& X2) {
  CommScope cs(X.grid);
  DevMat o, none;
  if (!isr_chain_on(X, X2) || !isr_chain_local(X, X2, 3, 0.0, 0.0, 0.0, o, none)) return false;
  X.loc = std::move(o);
  return true;
}
bool ps_isr_chain_step(const PSMatrix& X, const PSMatrix& X2, int order, double a, double b, double c, PSMatrix& Out1, PSMatrix& Out2) {
  CommScope cs(X.grid);
  if ((order != 5 && order != 3) || options().isr_chain == 0 || !slab_on() || X.cplx != X2.cplx || !session_takes(X.cplx) || !same_dim({&X, &X2}) ||
      !all_distinct({&X, &X2, &Out1, &Out2}))
    return false;
  unblock({&X, &X2});
  DevMat q, p;
  if (!isr_chain_local(X, X2, order, a, b, c, q, p)) return false;
  pack(q);
  install_like(Out1, X, X.cplx, std::move(q));
  if (order == 5) {
    pack(p);
    install_like(Out2, X, X.cplx, std::move(p));
  }
  return true;
}

long long* hpcp_step_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
namespace {
// MatrixTrace of the local panel of a matrix that is not in block form: ps_trace without its sum over the ranks
double trace_local(const PSMatrix& A) {
  unblock({&A});
  if (slab_on() && A.loc.expanded() && !A.cplx) {
    double v = 0.0;
    if (slab_trace(A.loc, A.c0, &v)) {
      g_slab_counts[2] += 1;
      return v;
    }
    slab_refused({&A});
  } else if (complex_passes_on(options().complex_scale_fold, {&A}) && A.loc.expanded() && !labelled(A)) {
    // (option complex_scale_fold: MatrixTrace of a complex slab-form matrix in a complex session is the pass over its runs, the sum
    // the loop's fused passes return -- every trace(X) of the loop on an X in slab form is then summed in one order, fused or not)
    double v = 0.0;
    if (slab_dot_trace_c(A.loc, nullptr, A.c0, nullptr, &v)) {
      g_slab_counts[2] += 1;
      return v;
    }
    slab_pack_if({&A});
  } else {
    slab_pack_if({&A});
  }
  return trace(A.loc, A.c0);
}
// the gates of the fused update (isr_chain_on for three merged operands and WH): a step they keep out is neither fused nor refused
bool hpcp_update_on(const PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, const PSMatrix& WH) {
  return options().hpcp_step != 0 && slab_on() && !D1.cplx && !DDH.cplx && !D2DH.cplx && !WH.cplx && same_dim({&D1, &DDH, &D2DH, &WH}) &&
         all_distinct({&D1, &DDH, &D2DH}) && !blk_any({&D1, &DDH, &D2DH, &WH}) && !WH.loc.blocked() &&
         (D1.loc.expanded() || DDH.loc.expanded() || D2DH.loc.expanded()) && !labelled(D1) && !labelled(DDH) && !labelled(D2DH) && !labelled(WH);
}
// the operands into slab form where they are, as ps_axpby and ps_dot do before their kernels.  *gated: what cannot be fused without
// being a refusal -- alignments that differ, a WH that is neither a zero-free slab form nor a read-only view.  Complex operands:
// WH may become a read-only view (stored zeros, option stored_zero_views), the merged operands may not
bool hpcp_enter(bool cplx, const PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, const PSMatrix& WH, bool* gated) {
  auto merged = [cplx](const PSMatrix& M) { return cplx ? slab_enter_c(mut(M), nullptr, false) : slab_enter(mut(M)); };
  *gated = false;
  if (!(cplx ? slab_enter_c(mut(WH)) : slab_enter(mut(WH))) || !(WH.loc.zero_free == 1 || WH.loc.slab->origin)) { *gated = true; return false; }
  if (!merged(D1) || !merged(DDH) || !merged(D2DH)) return false;
  if (D1.loc.slab->row_pad != DDH.loc.slab->row_pad || D1.loc.slab->row_pad != D2DH.loc.slab->row_pad) { *gated = true; return false; }
  return true;
}
bool hpcp_sigma_ok(double sigma) { return sigma != 0.0 && std::isfinite(sigma); }
// Option complex_hpcp: the two passes on COMPLEX operands, one rank, inside a session that takes complex operands.  The gates of
// complex TRS4 (complex_passes_on) and: no labelled slab form, distinct operands.  A pass they keep out is neither fused nor refused
bool chpcp_on(std::initializer_list<const PSMatrix*> ms) {
  if (!complex_passes_on(options().complex_hpcp, ms) || !all_distinct(ms)) return false;
  for (const PSMatrix* m : ms)
    if (labelled(*m)) return false;
  return true;
}
// the fused update past its gates, operands of one kind: the new D1 and DH in slab form and this rank's energy in e[0]; false: refused
// (counted) or gated.  A complex update counts in complex_hpcp_counts(), a real one in hpcp_step_counts()
bool hpcp_update_local(bool cplx, const PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, double sigma, const PSMatrix& WH, DevMat& o,
                       DevMat& h, double e[2]) {
  long long* counts = cplx ? complex_hpcp_counts() : hpcp_step_counts();
  bool gated = false;
  if (!hpcp_sigma_ok(sigma) || !hpcp_enter(cplx, D1, DDH, D2DH, WH, &gated) ||
      !(cplx ? slab_hpcp_update_c : slab_hpcp_update)(D1.loc, DDH.loc, D2DH.loc, sigma, WH.loc, D1.c0, o, h, &e[0])) {
    if (!gated) counts[2] += 1;
    return false;
  }
  g_slab_counts[1] += 4;   // two merges into D1; the copy and the identity's merge of DH (a complex update counts as the real one)
  g_slab_counts[2] += 2;   // the scaling of DH, the dot
  counts[1] += 1;
  return true;
}
bool chpcp_traces(const PSMatrix& DDH, const PSMatrix& D2DH, double out[2]) {
  double t[2] = {0.0, 0.0};
  if (!slab_hpcp_traces_c(DDH.loc, D2DH.loc, DDH.c0, t)) {
    complex_hpcp_counts()[2] += 1;
    return false;
  }
  g_slab_counts[2] += 2;
  complex_hpcp_counts()[0] += 1;
  out[0] = t[0];
  out[1] = t[1];
  return true;
}
}  // namespace
long long* complex_hpcp_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
bool ps_hpcp_traces(const PSMatrix& DDH, const PSMatrix& D2DH, double out[2]) {
  CommScope cs(DDH.grid);
  if (DDH.cplx || D2DH.cplx)   // (option complex_hpcp; one rank: no reduction)
    return chpcp_on({&DDH, &D2DH}) && DDH.loc.expanded() && D2DH.loc.expanded() && chpcp_traces(DDH, D2DH, out);
  // (every gate here is the same on every rank: past them each rank enters ONE reduction, and a rank whose panels the kernel does
  // not take adds the partial sums it computes as ps_trace would)
  if (options().hpcp_step == 0 || g_slab_depth == 0 || DDH.cplx || D2DH.cplx || DDH.dim != D2DH.dim || &DDH == &D2DH || blk_any({&DDH, &D2DH}) ||
      (!world().active() && !slab_on()))
    return false;
  double t[2] = {0.0, 0.0};
  if (slab_on() && DDH.loc.expanded() && D2DH.loc.expanded() && slab_hpcp_traces(DDH.loc, D2DH.loc, DDH.c0, t)) {
    g_slab_counts[2] += 2;
    hpcp_step_counts()[0] += 1;
  } else {
    t[0] = trace_local(DDH);
    t[1] = trace_local(D2DH);
  }
  comm_allreduce_sum(t, 2);
  out[0] = t[0];
  out[1] = t[1];
  return true;
}
bool ps_hpcp_update(PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, double sigma, const PSMatrix& WH, PSMatrix& DH, double* energy) {
  CommScope cs(D1.grid);
  if (&DH == &D1 || &DH == &DDH || &DH == &D2DH || &DH == &WH) return false;
  const bool cplx = D1.cplx || DDH.cplx || D2DH.cplx || WH.cplx;   // (option complex_hpcp; one rank: no reduction)
  if (cplx ? !chpcp_on({&D1, &DDH, &D2DH, &WH}) || !(D1.loc.expanded() || DDH.loc.expanded() || D2DH.loc.expanded())
           : !hpcp_update_on(D1, DDH, D2DH, WH))
    return false;
  DevMat o, h;
  double e[2] = {0.0, 0.0};
  if (!hpcp_update_local(cplx, D1, DDH, D2DH, sigma, WH, o, h, e)) return false;
  install_like(DH, D1, cplx, std::move(h));
  D1.loc = std::move(o);
  // (the reduction of the dot this replaces, entry for entry: a rank that refused is in ps_dot's with its own partial sum)
  if (!cplx) comm_allreduce_sum(e, 2);
  *energy = e[0];
  return true;
}
bool ps_hpcp_update_step(const PSMatrix& D1, const PSMatrix& DDH, const PSMatrix& D2DH, double sigma, const PSMatrix& WH, PSMatrix& D1out,
                         PSMatrix& DHout, double* energy) {
  CommScope cs(D1.grid);
  if (!all_distinct({&D1, &DDH, &D2DH, &D1out, &DHout}) || !all_distinct({&WH, &D1out, &DHout})) return false;
  const bool cplx = D1.cplx && DDH.cplx && D2DH.cplx && WH.cplx;   // (option complex_hpcp, under the gates of the loop's call)
  if (cplx) {
    if (!chpcp_on({&D1, &DDH, &D2DH, &WH})) return false;
  } else {
    if (options().hpcp_step == 0 || !slab_on() || D1.cplx || DDH.cplx || D2DH.cplx || WH.cplx || !same_dim({&D1, &DDH, &D2DH, &WH}) || labelled(D1) ||
        labelled(DDH) || labelled(D2DH) || labelled(WH))
      return false;
    unblock({&D1, &DDH, &D2DH, &WH});
  }
  DevMat o, h;
  double e[2] = {0.0, 0.0};
  if (!hpcp_update_local(cplx, D1, DDH, D2DH, sigma, WH, o, h, e)) return false;
  pack(o);
  pack(h);
  install_like(D1out, D1, cplx, std::move(o));
  install_like(DHout, D1, cplx, std::move(h));
  if (!cplx) comm_allreduce_sum(e, 2);
  *energy = e[0];
  return true;
}
bool ps_hpcp_traces_step(const PSMatrix& DDH, const PSMatrix& D2DH, double out[2]) {
  CommScope cs(DDH.grid);
  if (DDH.cplx || D2DH.cplx) {   // (option complex_hpcp, under the gates of the loop's call)
    if (!chpcp_on({&DDH, &D2DH})) return false;
    if (!slab_enter_c(mut(DDH)) || !slab_enter_c(mut(D2DH))) {
      complex_hpcp_counts()[2] += 1;
      return false;
    }
    return chpcp_traces(DDH, D2DH, out);
  }
  if (options().hpcp_step == 0 || !slab_on() || !same_dim({&DDH, &D2DH}) || &DDH == &D2DH || labelled(DDH) || labelled(D2DH)) return false;
  unblock({&DDH, &D2DH});
  double t[2] = {0.0, 0.0};
  if (!slab_enter(mut(DDH)) || !slab_enter(mut(D2DH)) || !slab_hpcp_traces(DDH.loc, D2DH.loc, DDH.c0, t)) return false;
  comm_allreduce_sum(t, 2);
  out[0] = t[0];
  out[1] = t[1];
  g_slab_counts[2] += 2;
  hpcp_step_counts()[0] += 1;
  return true;
}

long long* pm_session_counts() {
  static long long counts[5] = {0, 0, 0, 0, 0};
  return counts;
}
long long* complex_pm_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// Option complex_pm: the PM passes on COMPLEX operands, one rank, inside a session that takes complex operands.  The gates of
// complex TRS4 (complex_passes_on) and: distinct operands, none labelled.  A pass they keep out is neither fused nor refused
bool cpm_on(std::initializer_list<const PSMatrix*> ms) {
  if (!complex_passes_on(options().complex_pm, ms) || !all_distinct(ms)) return false;
  for (const PSMatrix* m : ms)
    if (labelled(*m)) return false;
  return true;
}
}  // namespace
bool ps_pm_sigma(const PSMatrix& X, const ZeroList& Z, const PSMatrix& X2, double threshold, double* trace_value, double* dot_value,
                 bool* gated) {
  CommScope cs(X.grid);
  if (gated) *gated = false;
  if (X.cplx || X2.cplx) {   // (option complex_pm; one rank: no reduction)
    if (!cpm_on({&X, &X2})) {
      if (gated) *gated = true;
      return false;
    }
    // (a read-only view -- a starting iterate that stores a zero -- and an iterate a product left in compressed columns are refused)
    double s[2] = {0.0, 0.0};
    if (!X.loc.expanded() || !X2.loc.expanded() || !slab_pm_sigma_c(X.loc, Z, X2.loc, threshold, X.c0, s)) return false;
    *trace_value = s[0];
    *dot_value = s[1];
    g_slab_counts[2] += 1;
    complex_pm_counts()[0] += 1;
    return true;
  }
  double t[3] = {0.0, 0.0, 0.0};
  const bool ok = slab_on() && !X.cplx && !X2.cplx && !blk_any({&X, &X2}) && X.loc.expanded() && X2.loc.expanded() &&
                  slab_pm_sigma(X.loc, Z, X2.loc, threshold, X.c0, t);
  if (world().active()) {
    // (a session across ranks: the decision is collective -- the sums and "some rank declined" in one reduction)
    if (!ok) { t[0] = t[1] = 0.0; t[2] = 1.0; }
    comm_allreduce_sum(t, 3);
    if (t[2] != 0.0) return false;
  } else if (!ok) {
    return false;
  }
  *trace_value = t[0];
  *dot_value = t[1];
  g_slab_counts[2] += 1;
  pm_session_counts()[0] += 1;
  return true;
}
bool ps_pm_update(PSMatrix& X, ZeroList& Z, const PSMatrix& X2, const PSMatrix& X3, double a1, double a2, double a3, double threshold) {
  CommScope cs(X.grid);
  DevMat R;
  ZeroList zn;
  if (X.cplx || X2.cplx || X3.cplx) {   // (option complex_pm; one rank.  Its own books: pm_session_counts() never counts a complex pass)
    if (cpm_on({&X, &X2, &X3}) && X.loc.expanded() && X2.loc.expanded() && X3.loc.expanded() &&
        slab_pm_update_c(X.loc, Z, X2.loc, X3.loc, a1, a2, a3, threshold, R, zn)) {
      X.loc = std::move(R);
      Z = std::move(zn);
      bump_matrix_value_epoch();
      g_slab_counts[1] += 2;
      complex_pm_counts()[1] += 1;
      complex_pm_counts()[2] += Z.count;
      return true;
    }
  } else if (slab_on() && !blk_any({&X, &X2, &X3}) && X.loc.expanded() && X2.loc.expanded() && X3.loc.expanded() &&
             slab_pm_update(X.loc, Z, X2.loc, X3.loc, a1, a2, a3, threshold, R, zn)) {
    X.loc = std::move(R);
    Z = std::move(zn);
    bump_matrix_value_epoch();
    g_slab_counts[1] += 2;
    pm_session_counts()[1] += 1;
    pm_session_counts()[2] += Z.count;
    pm_session_counts()[4] = std::max<long long>(pm_session_counts()[4], Z.count);
    return true;
  }
  // this rank cannot: its iterate as compressed columns hold it, and the two merges there (they are local to the panel)
  g_slab_counts[3] += 1;
  ps_pm_materialise(X, Z);
  unblock({&X2, &X3});
  DevMat t2, t3;
  axpby(columns_of(X2, t2), X.loc, a2, a1, threshold, nullptr, nullptr);
  axpby(columns_of(X3, t3), X.loc, a3, 1.0, threshold, nullptr, nullptr);
  return false;
}
void ps_pm_materialise(PSMatrix& X, ZeroList& Z) {
  CommScope cs(X.grid);
  ps_slab_leave(X);
  insert_stored_zeros(X.loc, Z);
  Z.clear();
}

void ps_copy_axpby(const PSMatrix& B, const PSMatrix& A, PSMatrix& Out, double alpha, double beta, double threshold) {
  CommScope cs(B.grid);
  if (blk_any({&A, &B}) && blk_kinds(A, B) && &A != &B && &Out != &A && &Out != &B) {
    ps_copy(B, Out);
    ps_axpby(A, Out, alpha, beta, threshold);
    return;
  }
  unblock({&A, &B});
  if (slab_on() && (A.loc.expanded() || B.loc.expanded()) && A.cplx == B.cplx && session_takes(A.cplx) && &A != &B && &Out != &A && &Out != &B &&
      A.dim == B.dim) {
    const SlabKind& k = slab_kind(A.cplx);
    DevMat R;
    const long long declined = slab_view_counts()[3];
    if (k.enter(mut(A)) && k.enter(mut(B)) && k.axpby_to(A.loc, B.loc, R, alpha, beta, threshold)) {
      g_slab_counts[1] += 1;
      install(Out, B.grid, B.dim, A.cplx, B.c0, B.c1, std::move(R));
      return;
    }
    if (slab_view_counts()[3] != declined) {
      slab_refused_view_merge();
      DevMat tmp;
      const DevMat& Ac = columns_of(A, tmp);
      R = is_view(B) ? B.loc.slab->origin->clone() : packed_copy(B.loc);
      axpby(Ac, R, alpha, beta, threshold, nullptr, nullptr);
      install(Out, B.grid, B.dim, A.cplx, B.c0, B.c1, std::move(R));
      return;
    }
    slab_refused({&A, &B});
  }
  ps_copy(B, Out);
  if (beta == 1.0) ps_increment(A, Out, alpha, threshold);
  else ps_axpby(A, Out, alpha, beta, threshold);
}

void ps_axpby_dot(const PSMatrix& A, PSMatrix& B, double alpha, double beta, double threshold, const PSMatrix& D, double out[4],
                  bool want_trace) {
  CommScope cs(A.grid);
  out[2] = out[3] = 0.0;
  if (A.cplx != B.cplx || A.cplx != D.cplx || &A == &B) {  // mixed types: unfused sequence
    ps_scale(B, beta);
    ps_increment(A, B, alpha, threshold);
    ps_dot(B, D, out);
    if (want_trace) out[2] = ps_trace(B);
    return;
  }
  axpby(A.loc, B.loc, alpha, beta, threshold, &D.loc, out, want_trace ? &out[2] : nullptr, B.c0);
  comm_allreduce_sum(out, want_trace ? 3 : 2);
}

namespace {
void dev_allreduce4(double* d) { world().tr->allreduce(d, 4, true, 0); }

// One TRS2 step of a rank whose panel is in slab form (kernels.hpp SlabForm): the halo travels as dense column runs
// (8 bytes per row of a column's span, no row ids, no offsets: every rank derives the layout from the all-gathered
// column extents), the run records of the kernel address the received runs where they land, the multiplier tiles are
// local.  Protocol, all on the engine stream with ONE host synchronisation: (1) ONE all-gather of a record per rank:
// request (first / last row of the panel, nnz), packed extents, prefix sums of the spans; (2) a kernel
// derives who sends how many doubles to whom, one read-back (PanelExchange prepare, fetch -- or left by the step before);
// (3) the runs of the requested columns are packed per requester and exchanged in one send / recv group (exchange);
// (4) layout kernel (halo), then slab_step.  Collective: every rank calls it.
// Returns this rank's success; the result is in fu.result (the caller installs it when all ranks succeeded).
bool slab_exchange_and_step(PSMatrix& B, SlabFusion& fu, double threshold, SlabReduce& red, bool* owed_prefetch) {
  static const bool step_times = std::getenv("NTPOLY_AMD_DEBUG_STEPTIME") != nullptr;   // (host clock of a panel step's phases, rank 0)
  const auto st0 = std::chrono::steady_clock::now();
  auto st_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - st0).count(); };
  double st_prep = 0, st_xchg = 0;
  const long long syncs_before = host_sync_count();
  const int P = world().nranks, me = world().rank;
  const int32_t dim = B.dim;
  const bool with_counts = options().time_kernels != 0;
  const bool ahead = options().exchange_ahead != 0 && exchange_fits_fetch(P);
  // the preparation: left behind by the step that produced this iterate, or made (and read back) here
  std::unique_ptr<PanelExchange> pe;
  // (matched by ALLOCATION, not by address: the allocator hands a freed address to the next matrix of the size, and a hit
  // decided from an address could differ between ranks -- one rank skipping an all-gather the others enter.  An allocation
  // serial names one buffer of one step's result; the steps are collective, so either every rank holds the preparation
  // of this iterate or none does)
  if (g_pending_exchange && g_pending_exchange->owner == B.loc.slab->val.p && g_pending_exchange->owner_serial != 0 &&
      g_pending_exchange->owner_serial == dev_alloc_serial(B.loc.slab->val.p) && g_pending_exchange->dim == dim && g_pending_exchange->P == P &&
      g_pending_exchange->with_counts == with_counts) {
    pe = std::move(g_pending_exchange);
    g_exchange_prefetched += 1;
  } else {
    g_pending_exchange.reset();
    pe.reset(new PanelExchange());
    pe->prepare(B.loc, nullptr, false, true, dim, nullptr);
    pe->fetch();
  }
  st_prep = st_ms();
  exchange_stats().host_syncs += host_sync_count() - syncs_before;   // (the exchange's own: measured in sync_stream)
  exchange_stats().exchanges += 1;
  int64_t nnz_global = 0;
  for (int q = 0; q < P; ++q) nnz_global += pe->req[(size_t)4 * q + 2];
  pe->exchange(B.loc, B.c0);
  st_xchg = st_ms();
  if (pe->kmax < pe->kmin) {   // (an empty panel: nothing to multiply; the caller's consensus takes the other path)
    if (ahead) *owed_prefetch = true;
    return false;
  }
  // (every rank packs with the alignment of its panel: the same option everywhere)
  SlabHalo halo = pe->halo(B.loc, std::max(1, B.loc.slab->row_pad));
  red.allreduce = &dev_allreduce4;
  halo.reduce = &red;
  // the NEXT step's preparation, from this step's result, on this step's read-back (option exchange_ahead)
  std::unique_ptr<PanelExchange> next;
  if (ahead) {
    halo.before_fetch = [&](const DevMat& R, const long long* d_nnz, ScalarFetch& f) {
      next.reset(new PanelExchange());
      next->prepare(R, nullptr, false, true, dim, d_nnz);
      next->add_to(f);
    };
  }
  const bool ok = slab_step(B.loc, fu, threshold, dense_branch(dim, nnz_global, nnz_global), &halo);
  if (step_times && me == 0)
    std::fprintf(stderr, "[panel step] preparation %.3f ms (%s), halo exchange %.3f ms (%lld doubles out, %lld in), step %.3f ms\n", st_prep,
                 g_exchange_prefetched ? "left by the step before or made" : "made", st_xchg - st_prep, (long long)pe->soff[(size_t)P],
                 (long long)pe->zoff[(size_t)P], st_ms() - st_xchg);
  if (ahead && !next) *owed_prefetch = true;   // (this rank gave up before its kernel: it owes the others the all-gather)
  if (ok && next) g_pending_exchange = std::move(next);
  return ok;
}

// the fused epilogue of a TRS2 step (kernels.hpp SlabFusion; panel_c0 >= 0: B is a column panel of the iterate)
SlabFusion trs2_fusion(int mode, double am, double bm, double threshold, const PSMatrix& D, int32_t col_offset, int32_t panel_c0) {
  SlabFusion fu;
  fu.mode = mode;
  fu.am = am;
  fu.bm = bm;
  fu.threshold = threshold;
  fu.D = &D.loc;
  fu.col_offset = col_offset;
  fu.panel_c0 = panel_c0;
  return fu;
}
// energy and trace of a step whose fusion is done
void fusion_scalars(const SlabFusion& fu, double out[4]) {
  out[0] = fu.dot;
  out[1] = 0.0;
  out[2] = fu.trace;
}

// TRS2 step across ranks with the fused kernel (mode 1: X <- X*X, mode 2: X <- 2X - X*X; energy and trace in out).
// true: done on every rank.  false: nothing changed (the panel is in compressed columns again), the caller runs
// the separate passes.  Collective.
bool dist_fused_step(PSMatrix& B, int mode, double threshold, const PSMatrix& D, double out[4]) {
  if (!B.loc.expanded()) return false;
  const int P = world().nranks;
  SlabFusion fu = trs2_fusion(mode, -1.0, 2.0, threshold, D, B.c0, B.c0);
  SlabReduce red;
  bool owed_prefetch = false;
  slab_exchange_and_step(B, fu, threshold, red, &owed_prefetch);   // (this rank's success is in the sums)
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (red.done) {   // the sums came back with the step's totals
    for (int q = 0; q < 4; ++q) v[q] = red.reduced[q];
  } else {          // this rank gave up before its kernel: it still owes the other ranks the collective
    comm_allreduce_sum(v, 4);
  }
  // ... and the all-gather of the next step's preparation, which the others will discard
  if (owed_prefetch && !red.done) owed_allgather(B.dim);
  if (v[3] != (double)P) g_pending_exchange.reset();
  if (v[3] == (double)P) {
    B.loc = std::move(fu.result);
    out[0] = v[0];
    out[1] = 0.0;
    out[2] = v[2];
    out[3] = 0.0;
    return true;
  }
  pack(B.loc);   // (some rank could not: every rank repeats the step on the unfused, equally collective path)
  return false;
}

// fused TRS2 steps across ranks: real operands, no process slices, no block-order solve (band_scope.cpp: its panel products
// take the block path of multiply_panel)
bool fused_across_ranks(const PSMatrix& B, const PSMatrix& D) {
  return world().active() && options().fused_update != 0 && options().loose_iterates != 0 && !B.cplx && !D.cplx &&
         !(B.grid && B.grid->num_slices > 1) && !block_scope_active();
}
// A fused TRS2 step across ranks from compressed panels: the product of the gathered halo with the panel, with the fused
// epilogue fu (energy, trace, slab form) where the kernel takes it -- otherwise `separate` finishes this rank's step from the
// product in AB / L (L == nullptr: no loose product wanted).  fu.mode == 0: the product only, false -- the caller's separate
// passes follow.  true: the step is done on every rank, out holds the sums.  nnz: this panel's entries, for the dense-branch
// rule.  Collective.
template <class Separate>
bool panel_step_from_columns(PSMatrix& B, int64_t nnz, SlabFusion& fu, double threshold, double out[4], DevMat& AB, LooseProduct* L,
                             Separate separate) {
  int64_t nz[2] = {nnz, nnz};
  HaloExchange hx;
  gather_needed_begin(hx, B, B.loc, nz, false);
  hx.finish();
  const ColRange need{hx.kmin, hx.kmax + 1};
  spgemm(hx.full, B.loc, AB, 1.0, threshold, dense_branch(B.dim, nz[0], nz[1]), L, &need, fu.mode ? &fu : nullptr);
  if (!fu.mode) return false;
  // the ranks must agree on the form of the iterate (the next step's exchange depends on it): slab form only if
  // every rank's kernel produced it
  if (fu.done) fusion_scalars(fu, out);
  else separate();
  out[3] = fu.done ? 1.0 : 0.0;
  comm_allreduce_sum(out, 4);
  if (fu.done) {
    B.loc = std::move(fu.result);
    if (out[3] != (double)world().nranks) pack(B.loc);
  }
  out[3] = 0.0;
  return true;
}
}  // namespace

// TRS2, sigma > 0 (DensityMatrixSolversModule.F90:388-396): X2 = X*X; X = 2X - X2; energy = dot(X, D).  When the
// register-slab kernel computes X*X the product is never compacted: the merge kernel reads it from its slots.
namespace {
// a fused TRS2 step reads the iterate's multiplier tiles; an iterate that the slab algebra left in slab form (runs only,
// or the read-only view of a matrix with stored zeros) goes back to compressed columns first
void trs2_iterate_form(PSMatrix& B) {
  if (!B.loc.expanded()) return;
  // (the MFMA tile kernel on one rank builds its multiplier tiles from the runs; the unfused loop and the panel steps
  // read them from memory)
  const bool need_tiles = options().spgemm_fma != 1 || world().active();
  const bool no_tiles = B.loc.slab->tiles.p == nullptr || B.loc.slab->tile_off.p == nullptr;
  if (B.loc.slab->origin || (need_tiles && no_tiles)) pack(B.loc);
}
}  // namespace

namespace {
// TRS2 steps of an iterate without run structure: block form from step to step (spgemm_block.hip), one rank, real
bool trs2_block(PSMatrix& B, int mode, double threshold, const PSMatrix& D, double out[4]) {
  if (world().active() || B.cplx || D.cplx || (B.grid && B.grid->num_slices > 1) || options().fused_update == 0 || options().loose_iterates == 0) {
    if (B.loc.blocked()) pack(B.loc);
    return false;
  }
  if (!B.loc.blocked() && (B.loc.expanded() || B.loc.loose() || !B.loc.block_hint)) return false;
  if (trs2_block_step(B.loc, mode, threshold, dense_branch(B.dim, B.loc.nnz, B.loc.nnz), D.loc, out)) return true;
  if (B.loc.blocked()) pack(B.loc);
  return false;
}
}  // namespace

namespace {
// Complex TRS2 steps that keep the iterate out of compressed columns (option complex_density; one rank, FMA arithmetic,
// complex_tile, complex_sessions):
//  - run-like iterates in complex SLAB form: X*X on the complex tile kernel (slab_multiply_c), 2X - X*X by the complex merge of
//    the slab algebra (the AddSparseVectors rules with the threshold on the modulus), then ONE pass for the energy Re sum conj(X) D
//    and the trace Re sum X_ii (slab_extra.hip k_sa_dot_trace_c);
//  - iterates without runs (a complex lattice) in complex BLOCK form (block_complex, block_path): X*X on k_bs_numeric_c kept in
//    block form, 2X - X*X by the complex block merge (k_bs_merge on complex tiles), energy and trace by block_dot_trace.
// An iterate the slab form cannot hold (stored zeros) runs its step the old way and the next step tries again.  A Hamiltonian
// whose iterates neither form takes is remembered (by identity) and its later steps go the old way at once.
struct CtrsOff {
  const DevMat* d = nullptr;
  const double* val = nullptr;
  int64_t nnz = -1;
};
CtrsOff g_ctrs2_off;
bool ctrs2_off_for(const PSMatrix& D) { return g_ctrs2_off.d == &D.loc && g_ctrs2_off.val == D.loc.val.p && g_ctrs2_off.nnz == D.loc.nnz; }
void ctrs2_set_off(const PSMatrix& D) { g_ctrs2_off.d = &D.loc; g_ctrs2_off.val = D.loc.val.p; g_ctrs2_off.nnz = D.loc.nnz; }
bool complex_trs2_block(PSMatrix& B, int mode, double threshold, bool dense_rule, const PSMatrix& D, double out[4]) {
  if (!complex_forms_ok() || options().block_path == 0 || options().block_complex == 0 || B.loc.expanded() || D.loc.expanded()) return false;
  DevMat P;
  BlockInfo info;
  if (!spgemm_block(B.loc, B.loc, P, 1.0, threshold, dense_rule, &info, nullptr, nullptr, true)) return false;
  if (!P.blocked()) {   // (an empty product: no block form to carry on with)
    if (B.loc.blocked()) pack(B.loc);
    return false;
  }
  if (mode == 2) {
    if (!block_axpby(P, B.loc, -1.0, 2.0, threshold)) {
      complex_fusion_counts()[2] += 1;
      if (B.loc.blocked()) pack(B.loc);
      return false;
    }
  } else {
    B.loc = std::move(P);
  }
  double dot[2] = {0.0, 0.0}, tr = 0.0;
  if (!block_dot_trace(B.loc, D.loc, dot, &tr)) {   // (B is the new iterate now: the energy on compressed columns)
    pack(B.loc);
    dot_trace(B.loc, D.loc, out, &out[2], B.c0);
    out[1] = 0.0;
    complex_fusion_counts()[mode == 1 ? 0 : 1] += 1;
    return true;
  }
  complex_fusion_counts()[mode == 1 ? 0 : 1] += 1;
  out[0] = dot[0];
  out[1] = 0.0;
  out[2] = tr;
  return true;
}
bool complex_trs2_step(PSMatrix& B, int mode, double threshold, const PSMatrix& D, double out[4]) {
  if (!B.cplx || !D.cplx || options().complex_density == 0 || options().complex_sessions == 0 || options().spgemm_fma != 1 ||
      options().complex_tile == 0 || options().spgemm_variant >= 0 || options().spgemm_force_bin > 0 || world().active() ||
      (B.grid && B.grid->num_slices > 1) || block_scope_active())
    return false;
  if (B.loc.loose() || D.loc.blocked() || D.loc.loose() || B.dim != B.loc.cols || B.loc.nnz == 0 ||
      D.loc.rows != B.loc.rows || D.loc.cols != B.loc.cols || (D.loc.expanded() && (D.loc.slab->labelled() || D.loc.slab->origin)))
    return false;
  if (ctrs2_off_for(D)) return false;
  const bool dense_rule = dense_branch(B.dim, B.loc.nnz, B.loc.nnz);
  if (B.loc.blocked()) return complex_trs2_block(B, mode, threshold, dense_rule, D, out);
  if (!B.loc.expanded()) {
    bool not_runs = false;
    if (!slab_enter_c(B.loc, &not_runs, false)) {   // (no view iterate: stored zeros refuse as ever)
      if (!not_runs) return false;   // (stored zeros: this step the old way)
      if (complex_trs2_block(B, mode, threshold, dense_rule, D, out)) return true;
      ctrs2_set_off(D);
      return false;
    }
  }
  if (!sa_operand_c(B.loc) || B.loc.zero_free != 1) {
    pack(B.loc);
    return false;
  }
  DevMat P;
  bool ok = slab_multiply_c(B.loc, B.loc, P, 1.0, threshold, dense_rule);
  if (!ok) ctrs2_set_off(D);   // (the product's geometry does not fit the complex tile kernel: it will not next time either)
  if (ok && mode == 2) ok = slab_axpby_c(P, B.loc, -1.0, 2.0, threshold);   // (refused: B is the iterate the step started from)
  if (!ok) {
    complex_fusion_counts()[2] += 1;
    pack(B.loc);
    return false;
  }
  if (mode == 1) B.loc = std::move(P);
  double dot[2] = {0.0, 0.0}, tr = 0.0;
  slab_dot_trace_c(B.loc, &D.loc, B.c0, dot, &tr);   // (takes every operand admitted above)
  complex_fusion_counts()[mode == 1 ? 0 : 1] += 1;
  out[0] = dot[0];
  out[1] = 0.0;
  out[2] = tr;
  return true;
}
}  // namespace

void trs2_complex_reset() { g_ctrs2_off = CtrsOff(); }

void ps_square_update_dot(PSMatrix& B, PSMatrix& scratch, double threshold, const PSMatrix& D, double out[4], bool want_trace) {
  CommScope cs(D.grid);
  out[2] = out[3] = 0.0;
  if (complex_trs2_step(B, 2, threshold, D, out)) return;
  if (trs2_block(B, 2, threshold, D, out)) return;
  trs2_iterate_form(B);
  // (process slices: the K-split sums of ps_multiply; a solve in a block order across ranks, band_scope.cpp: the panel product
  // on the block path of multiply_panel)
  if (B.cplx || D.cplx != B.cplx || (B.grid && B.grid->num_slices > 1) || (block_scope_active() && world().active())) {
    pack(B.loc);
    ps_multiply(B, B, scratch, 1.0, 0.0, threshold);
    ps_axpby_dot(scratch, B, -1.0, 2.0, threshold, D, out, want_trace);
    return;
  }
  const int64_t nnz = B.loc.nnz;   // (for the dense-branch rule: the iterate as the step found it)
  LooseProduct L;
  DevMat AB;
  // the merge of the product in compressed columns (no loose product): scratch holds it
  auto merge_packed = [&](double* trace) {
    install(scratch, B.grid, B.dim, B.cplx, B.c0, B.c1, std::move(AB));
    axpby(scratch.loc, B.loc, -1.0, 2.0, threshold, &D.loc, out, trace, B.c0);
  };
  // one rank: the iterate may stay loose from step to step (kernels.hpp, axpby keep_loose)
  const bool keep_loose = !world().active() && options().loose_iterates != 0;
  const bool dist_fused = fused_across_ranks(B, D);
  if (dist_fused && dist_fused_step(B, 2, threshold, D, out)) return;
  if (!keep_loose) pack(B.loc);
  if (world().active()) {
    // (as on one rank; B is the panel [c0, c1) of the iterate whose needed columns the gathered operand holds)
    SlabFusion fu = trs2_fusion(dist_fused ? 2 : 0, -1.0, 2.0, threshold, D, B.c0, B.c0);
    const bool done = panel_step_from_columns(B, nnz, fu, threshold, out, AB, &L, [&] {
      if (L.valid) axpby(L, B.loc, -1.0, 2.0, threshold, &D.loc, out, &out[2], B.c0, nullptr, false);
      else merge_packed(&out[2]);
    });
    if (done) return;
  } else {
    const bool dense_rule = dense_branch(B.dim, nnz, nnz);
    // the whole update inside the multiply's epilogue when the register-slab kernel takes it
    SlabFusion fu = trs2_fusion(keep_loose && options().fused_update ? 2 : 0, -1.0, 2.0, threshold, D, B.c0, -1);
    // an operand without run structure may hide a band under its labels (kernels.hpp relabel_enter)
    if (fu.mode && !B.loc.expanded() && !B.loc.loose()) relabel_enter(B.loc, D.loc);
    if (B.loc.expanded() && B.loc.slab->labelled()) {
      fu.D = relabelled_operand(D.loc);
      if (!fu.D) {   // (D changed under the loop: back to the caller's labels)
        pack(B.loc);
        fu.D = &D.loc;
      }
    }
    if (B.loc.expanded()) {   // the iterate is in the kernel's own form already: no preparation pass at all
      if (fu.mode && slab_step(B.loc, fu, threshold, dense_rule)) {
        fusion_scalars(fu, out);
        return;
      }
      if (B.loc.slab->labelled()) relabel_giveup(D.loc);
      pack(B.loc);
      fu.D = &D.loc;
    }
    spgemm(B.loc, B.loc, AB, 1.0, threshold, dense_rule, &L, nullptr, fu.mode ? &fu : nullptr);
    if (fu.done) {
      B.loc = std::move(fu.result);
      fusion_scalars(fu, out);
      return;
    }
  }
  if (L.valid) {
    axpby(L, B.loc, -1.0, 2.0, threshold, &D.loc, out, want_trace ? &out[2] : nullptr, B.c0, nullptr, keep_loose);
  } else {
    pack(B.loc);
    merge_packed(want_trace ? &out[2] : nullptr);
  }
  if (last_spgemm_stats().block) B.loc.block_hint = 1;   // (the next step takes the iterate in block form: trs2_block)
  comm_allreduce_sum(out, want_trace ? 3 : 2);
}

// B <- B * B, out = dot(B_new, D) (+ trace(B_new)): the sigma < 0 step of TRS2.  On one rank with real operands the
// product stays loose (no compaction pass); otherwise multiply, swap and reduce as before.
void ps_square_dot(PSMatrix& B, PSMatrix& scratch, double threshold, const PSMatrix& D, double out[4], bool want_trace) {
  CommScope cs(D.grid);
  out[2] = out[3] = 0.0;
  if (complex_trs2_step(B, 1, threshold, D, out)) return;
  if (trs2_block(B, 1, threshold, D, out)) return;
  trs2_iterate_form(B);
  const bool keep_loose = !world().active() && options().loose_iterates != 0 && !B.cplx && !D.cplx &&
                          !(B.grid && B.grid->num_slices > 1);
  if (keep_loose &&
      square_keep_loose(B.loc, threshold, dense_branch(B.dim, B.loc.nnz, B.loc.nnz), D.loc, out, want_trace ? &out[2] : nullptr, B.c0))
    return;
  if (fused_across_ranks(B, D)) {
    if (dist_fused_step(B, 1, threshold, D, out)) return;
    // from compressed panels: the product with the fused epilogue (energy, trace, slab form) where the kernel takes it
    pack(B.loc);
    SlabFusion fu = trs2_fusion(1, 0.0, 0.0, 0.0, D, B.c0, B.c0);
    DevMat AB;
    panel_step_from_columns(B, B.loc.nnz, fu, threshold, out, AB, nullptr, [&] {
      B.loc = std::move(AB);
      dot_trace(B.loc, D.loc, out, &out[2], B.c0);
    });
    return;
  }
  pack(B.loc);
  ps_multiply(B, B, scratch, 1.0, 0.0, threshold);
  std::swap(B.loc, scratch.loc);  // B <- B*B; scratch is recomputed by the next multiply, so no copy
  if (last_spgemm_stats().block) B.loc.block_hint = 1;
  ps_dot_trace(B, D, out, want_trace);
}

// dot(A, B) and trace(A) from one pass
void ps_dot_trace(const PSMatrix& A, const PSMatrix& B, double out[4], bool want_trace) {
  CommScope cs(A.grid);
  unblock({&A, &B});
  out[2] = out[3] = 0.0;
  if (A.cplx != B.cplx) {
    ps_dot(A, B, out);
    if (want_trace) out[2] = ps_trace(A);
    return;
  }
  dot_trace(A.loc, B.loc, out, want_trace ? &out[2] : nullptr, A.c0);
  comm_allreduce_sum(out, want_trace ? 3 : 2);
}

void ps_pairwise(const PSMatrix& A, const PSMatrix& B, PSMatrix& C) {
  CommScope cs(A.grid);
  unblock({&A, &B});
  if (A.cplx != B.cplx) {
    PSMatrix Ac, Bc;
    ps_to_complex(A, Ac);
    ps_to_complex(B, Bc);
    ps_pairwise(Ac, Bc, C);
    return;
  }
  DevMat R;
  pairwise(A.loc, B.loc, R, false);
  install(C, A.grid, A.dim, A.cplx, A.c0, A.c1, std::move(R));
}

// DotMatrix_psr/psc (PSMatrixAlgebraModule.F90:387-410, distributed_algebra_includes/DotMatrix.f90):
// sum conj(A).B; fused, no Hadamard temporary.
namespace {
// DotMatrix of the local panels of two matrices that are not in block form: ps_dot without its sum over the ranks
void dot_local(const PSMatrix& A, const PSMatrix& B, double out[2]) {
  unblock({&A, &B});
  if (slab_on() && (A.loc.expanded() || B.loc.expanded()) && !A.cplx && !B.cplx) {
    // (a rank whose operands left slab form computes its share from compressed columns: the sum over the ranks follows either way)
    if (slab_enter(mut(A)) && slab_enter(mut(B)) && slab_dot(A.loc, B.loc, out)) {
      g_slab_counts[2] += 1;
      return;
    }
    slab_refused({&A, &B});
  } else {
    slab_pack_if({&A, &B});
  }
  if (A.cplx != B.cplx) {
    PSMatrix Ac, Bc;
    ps_to_complex(A, Ac);
    ps_to_complex(B, Bc);
    dot(Ac.loc, Bc.loc, out);
  } else {
    dot(A.loc, B.loc, out);
  }
}
// extra (optional): one more number summed over the ranks by the reduction the dot makes anyway
void ps_dot_with(const PSMatrix& A, const PSMatrix& B, double out[2], double* extra) {
  CommScope cs(A.grid);
  auto reduce = [&]() {
    if (!extra) { comm_allreduce_sum(out, 2); return; }
    double t[3] = {out[0], out[1], *extra};
    comm_allreduce_sum(t, 3);
    out[0] = t[0]; out[1] = t[1]; *extra = t[2];
  };
  if (blk_any({&A, &B}) && blk_kinds(A, B)) {
    double d[2] = {0.0, 0.0};
    // (the sum runs over the super-tiles of its first operand: the one in block form; sum conj(b) a = conj(sum conj(a) b))
    const bool swap = !A.loc.blocked();
    const bool ok = swap ? block_dot_trace(B.loc, A.loc, d, nullptr) : block_dot_trace(A.loc, B.loc, d, nullptr);
    if (ok) {
      g_block_counts[0] += 1;
      out[0] = d[0];
      out[1] = (swap && (A.cplx || B.cplx)) ? -d[1] : d[1];
      return;
    }
    g_block_counts[1] += 1;
  }
  dot_local(A, B, out);
  reduce();
}
}  // namespace
void ps_dot(const PSMatrix& A, const PSMatrix& B, double out[2]) { ps_dot_with(A, B, out, nullptr); }
double ps_pm_energy(const PSMatrix& X, const PSMatrix& WH, bool refused_here, bool* some_refused) {
  if (X.cplx && WH.cplx && !refused_here && &X != &WH && cpm_on({&X, &WH}) && X.loc.expanded() && sa_operand_c(X.loc)) {
    // (option complex_pm; one rank: one pass over X's runs and WH as it stands -- complex slab form, a read-only view, or compressed
    // columns --, as ps_trs4_energy takes it, where the dot below would pack X first)
    CommScope cs(X.grid);
    double dot[2] = {0.0, 0.0};
    if (slab_dot_trace_c(X.loc, &WH.loc, X.c0, dot, nullptr)) {
      g_slab_counts[2] += 1;
      *some_refused = false;
      return dot[0];
    }
  }
  double out[2], flag = refused_here ? 1.0 : 0.0;
  ps_dot_with(X, WH, out, &flag);
  *some_refused = flag != 0.0;
  return out[0];
}

double ps_trace(const PSMatrix& A) {
  CommScope cs(A.grid);  // MatrixTrace (distributed_algebra_includes/MatrixTrace.f90)
  if (blk_any({&A})) {
    double t = 0.0;
    if (block_dot_trace(A.loc, A.loc, nullptr, &t)) { g_block_counts[0] += 1; return t; }
    g_block_counts[1] += 1;
  }
  double t = trace_local(A);
  comm_allreduce_sum(&t, 1);
  return t;
}

long long* scale_fold_step_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
namespace {
// the gates of a fused ScaleAndFold call that are the same on every rank (X2: the fold branch's second operand, or none): a call
// they keep out is neither fused nor refused, and past them every rank enters ONE reduction
bool saf_gates(const PSMatrix& X, const PSMatrix* X2, const PSMatrix& WH) {
  if (options().scale_fold_step == 0 || g_slab_depth == 0 || X.cplx || WH.cplx || X.dim != WH.dim || &X == &WH || blk_any({&X, &WH})) return false;
  if (X2 && (X2->cplx || X2->dim != X.dim || X2 == &X || X2 == &WH || blk_any({X2}))) return false;
  return world().active() || slab_on();
}
// the operands into slab form where they are, as ps_axpby and ps_dot do before their kernels (hpcp_update_enter).  *gated: what
// cannot be fused on this rank without being a refusal -- a session that has given up slab form, a labelled slab form, in_loop:
// merged operands all in compressed columns, a WH that is neither a zero-free slab form nor a read-only view, alignments that differ
bool saf_enter(const PSMatrix& X, const PSMatrix* X2, const PSMatrix& WH, bool in_loop, bool* gated) {
  *gated = true;
  if (!slab_on() || labelled(X) || labelled(WH) || (X2 && labelled(*X2)) || WH.loc.blocked()) return false;
  if (in_loop && !X.loc.expanded() && !(X2 && X2->loc.expanded())) return false;
  if (!slab_enter(mut(WH)) || !(WH.loc.zero_free == 1 || WH.loc.slab->origin)) return false;
  *gated = false;
  if (!slab_enter(mut(X)) || (X2 && !slab_enter(mut(*X2)))) return false;
  if (X2 && X.loc.slab->row_pad != X2->loc.slab->row_pad) { *gated = true; return false; }
  return true;
}
// X2 given: the fold update into `out`; none: the sums of X as it stands.  sums = {dot, trace} of this rank's panel
bool saf_local(const PSMatrix& X, const PSMatrix* X2, double a, double b, const PSMatrix& WH, bool in_loop, DevMat& out, double sums[2]) {
  bool gated = false;
  const bool taken = std::isfinite(a) && std::isfinite(b) && saf_enter(X, X2, WH, in_loop, &gated) &&
                     (X2 ? slab_saf_update(X.loc, X2->loc, a, b, WH.loc, X.c0, out, &sums[0], &sums[1])
                         : slab_saf_dot_trace(X.loc, WH.loc, X.c0, &sums[0], &sums[1]));
  if (taken) {
    if (X2) g_slab_counts[1] += 1;   // the merge
    g_slab_counts[2] += 2;           // the dot, the next step's trace
    scale_fold_step_counts()[X2 ? 0 : 1] += 1;
  } else if (!gated) {
    scale_fold_step_counts()[2] += 1;
  }
  return taken;
}
// Option complex_scale_fold: the two passes on COMPLEX operands, one rank, inside a session that takes complex operands.  The gates
// of complex TRS4 (complex_passes_on) and: no labelled slab form, distinct operands.  A pass they keep out is neither fused nor refused
bool csaf_on(const PSMatrix& X, const PSMatrix* X2, const PSMatrix& WH) {
  const bool on = X2 ? complex_passes_on(options().complex_scale_fold, {&X, X2, &WH}) && all_distinct({&X, X2, &WH})
                     : complex_passes_on(options().complex_scale_fold, {&X, &WH}) && &X != &WH;
  return on && !labelled(X) && !labelled(WH) && !(X2 && labelled(*X2));
}
// the complex fold update past its gates (what the complex HPCP update takes: WH may become a read-only view, the merged operands
// may not), sums = {Re dot, trace}; false: refused (counted) or gated
bool csaf_update_local(const PSMatrix& X, const PSMatrix& X2, double a, double b, const PSMatrix& WH, DevMat& out, double sums[2]) {
  bool gated = false;
  const bool taken = [&] {
    if (!std::isfinite(a) || !std::isfinite(b)) return false;   // (refused before any operand is touched, as saf_local does)
    if (!slab_enter_c(mut(WH)) || !(WH.loc.zero_free == 1 || WH.loc.slab->origin)) { gated = true; return false; }
    if (!slab_enter_c(mut(X), nullptr, false) || !slab_enter_c(mut(X2), nullptr, false)) return false;
    if (X.loc.slab->row_pad != X2.loc.slab->row_pad) { gated = true; return false; }
    return slab_saf_update_c(X.loc, X2.loc, a, b, WH.loc, X.c0, out, &sums[0], &sums[1]);
  }();
  if (taken) {
    g_slab_counts[1] += 1;   // the merge (a complex update counts as the real one)
    g_slab_counts[2] += 2;   // the dot, the next step's trace
    complex_scale_fold_counts()[0] += 1;
  } else if (!gated) {
    complex_scale_fold_counts()[2] += 1;
  }
  return taken;
}
// the scale branch's pass on a complex X in slab form and WH as it stands (what ps_trs4_energy takes: complex slab form, a
// read-only view, or compressed columns -- stored zeros add exact zeros to the sum); false: refused (counted)
bool csaf_dot_trace_local(const PSMatrix& X, const PSMatrix& WH, double sums[2]) {
  double dot[2] = {0.0, 0.0}, t = 0.0;
  if (!sa_operand_c(X.loc) || !slab_dot_trace_c(X.loc, &WH.loc, X.c0, dot, &t)) {
    complex_scale_fold_counts()[2] += 1;
    return false;
  }
  g_slab_counts[2] += 2;   // the dot, the next step's trace
  complex_scale_fold_counts()[1] += 1;
  sums[0] = dot[0];
  sums[1] = t;
  return true;
}
}  // namespace
long long* complex_scale_fold_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
bool ps_saf_update(PSMatrix& X, const PSMatrix& X2, double a, double b, const PSMatrix& WH, double* dot, double* trace) {
  CommScope cs(X.grid);
  if (X.cplx || X2.cplx || WH.cplx) {   // (option complex_scale_fold; one rank: no reduction)
    DevMat o;
    double s[2] = {0.0, 0.0};
    if (!csaf_on(X, &X2, WH) || !(X.loc.expanded() || X2.loc.expanded()) || !csaf_update_local(X, X2, a, b, WH, o, s)) return false;
    X.loc = std::move(o);
    *dot = s[0];
    *trace = s[1];
    return true;
  }
  if (!saf_gates(X, &X2, WH)) return false;
  DevMat o;
  double s[2] = {0.0, 0.0};
  if (saf_local(X, &X2, a, b, WH, true, o, s)) {
    X.loc = std::move(o);
  } else {
    if (!world().active()) return false;
    // (across ranks: this rank runs the calls on its panel and brings the partial sums they compute to the one reduction)
    ps_axpby(X2, X, a, b, 0.0);
    dot_local(X, WH, s);
    s[1] = trace_local(X);
  }
  comm_allreduce_sum(s, 2);
  *dot = s[0];
  *trace = s[1];
  return true;
}
bool ps_saf_dot_trace(const PSMatrix& X, const PSMatrix& WH, double* dot, double* trace) {
  CommScope cs(X.grid);
  if (X.cplx || WH.cplx) {   // (option complex_scale_fold; one rank: no reduction)
    double s[2] = {0.0, 0.0};
    if (!csaf_on(X, nullptr, WH) || !X.loc.expanded() || !csaf_dot_trace_local(X, WH, s)) return false;
    *dot = s[0];
    *trace = s[1];
    return true;
  }
  if (!saf_gates(X, nullptr, WH)) return false;
  DevMat none;
  double s[2] = {0.0, 0.0};
  if (!saf_local(X, nullptr, 1.0, 1.0, WH, true, none, s)) {
    if (!world().active()) return false;
    dot_local(X, WH, s);
    s[1] = trace_local(X);
  }
  comm_allreduce_sum(s, 2);
  *dot = s[0];
  *trace = s[1];
  return true;
}
bool ps_saf_update_step(const PSMatrix& X, const PSMatrix& X2, double a, double b, const PSMatrix& WH, PSMatrix& Xout, double* dot, double* trace) {
  CommScope cs(X.grid);
  if (X.cplx || X2.cplx || WH.cplx) {   // (option complex_scale_fold, under the gates of the loop's call)
    DevMat o;
    double s[2] = {0.0, 0.0};
    if (!csaf_on(X, &X2, WH) || &Xout == &X || &Xout == &X2 || &Xout == &WH || !csaf_update_local(X, X2, a, b, WH, o, s)) return false;
    pack(o);
    install_like(Xout, X, true, std::move(o));
    *dot = s[0];
    *trace = s[1];
    return true;
  }
  if (!saf_gates(X, &X2, WH) || &Xout == &X || &Xout == &X2 || &Xout == &WH) return false;
  DevMat o;
  double s[2] = {0.0, 0.0};
  if (!saf_local(X, &X2, a, b, WH, false, o, s)) return false;
  pack(o);
  install(Xout, X.grid, X.dim, false, X.c0, X.c1, std::move(o));
  comm_allreduce_sum(s, 2);
  *dot = s[0];
  *trace = s[1];
  return true;
}
bool ps_saf_dot_trace_step(const PSMatrix& X, const PSMatrix& WH, double* dot, double* trace) {
  CommScope cs(X.grid);
  if (X.cplx || WH.cplx) {   // (option complex_scale_fold, under the gates of the loop's call)
    double s[2] = {0.0, 0.0};
    if (!csaf_on(X, nullptr, WH)) return false;
    if (!X.loc.expanded() && !slab_enter_c(mut(X), nullptr, false)) {
      complex_scale_fold_counts()[2] += 1;
      return false;
    }
    if (!csaf_dot_trace_local(X, WH, s)) return false;
    *dot = s[0];
    *trace = s[1];
    return true;
  }
  if (!saf_gates(X, nullptr, WH)) return false;
  DevMat none;
  double s[2] = {0.0, 0.0};
  if (!saf_local(X, nullptr, 1.0, 1.0, WH, false, none, s)) return false;
  comm_allreduce_sum(s, 2);
  *dot = s[0];
  *trace = s[1];
  return true;
}

namespace {
// MatrixNorm of the local panel of a matrix that is not in block form: ps_norm without its maximum over the ranks
double norm_local(const PSMatrix& A) {
  unblock({&A});
  if (slab_on() && A.loc.expanded()) {
    // (a complex operand outside a session that takes them is refused: the real slab_norm declines it untouched)
    double v = 0.0;
    if (session_takes(A.cplx) && slab_kind(A.cplx).norm(A.loc, &v)) {
      g_slab_counts[2] += 1;
      return v;
    }
    slab_refused({&A});
  } else {
    slab_pack_if({&A});
  }
  DevBuf<double> sums;
  column_abs_sums(A.loc, sums);
  return max_of(sums, (size_t)A.loc.cols);
}
}  // namespace
double ps_norm(const PSMatrix& A) {
  CommScope cs(A.grid);  // MatrixNorm: max column abs-sum; columns are local
  if (blk_any({&A})) {
    double v = 0.0;
    if (block_norm(A.loc, &v)) { g_block_counts[0] += 1; return v; }
    g_block_counts[1] += 1;
  }
  double n = norm_local(A);
  comm_allreduce_max(&n, 1);   // (columns are local: a rank whose slab form declines computed its part from compressed columns, every rank reduces once)
  return n;
}

long long* wom_session_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// the gates of a fused WOM pass that are the same on every rank: a call they keep out is neither fused nor refused, and past them
// every rank enters ONE reduction
bool wom_gates(std::initializer_list<const PSMatrix*> ms, const PSMatrix* out = nullptr) {
  if (options().wom_session < 2 || g_slab_depth == 0 || !all_distinct(ms) || !same_dim(ms) || blk_any(ms)) return false;
  for (const PSMatrix* m : ms)
    if (m->cplx || labelled(*m) || m == out) return false;
  return world().active() || slab_on();
}
// the Heun tail on this rank's panel into `out`, maxima = {err, err2} of the panel; false: refused (counted)
bool wom_heun_local(const PSMatrix& W, const PSMatrix& K0, const PSMatrix& K1, const PSMatrix& RK1, double step, double threshold, DevMat& out,
                    double maxima[2]) {
  const bool taken = std::isfinite(step) && std::isfinite(threshold) && slab_on() && slab_enter(mut(W)) && slab_enter(mut(K0)) &&
                     slab_enter(mut(K1)) && slab_enter(mut(RK1)) &&
                     slab_wom_heun(W.loc, K0.loc, K1.loc, RK1.loc, step, threshold, out, &maxima[0], &maxima[1]);
  if (taken) {
    g_slab_counts[1] += 7;   // the two copies and the merges into RK2 and the two differences
    g_slab_counts[2] += 2;   // the two norms
    wom_session_counts()[1] += 1;
  } else {
    wom_session_counts()[3] += 1;
  }
  return taken;
}
}  // namespace
bool ps_wom_heun(const PSMatrix& W, const PSMatrix& K0, const PSMatrix& K1, const PSMatrix& RK1, double step, double threshold, PSMatrix& RK2,
                 double* err, double* err2) {
  CommScope cs(W.grid);
  if (!wom_gates({&W, &K0, &K1, &RK1}, &RK2)) return false;
  DevMat o;
  double m[2] = {0.0, 0.0};
  if (wom_heun_local(W, K0, K1, RK1, step, threshold, o, m)) {
    install_like(RK2, W, false, std::move(o));
  } else {
    if (!world().active()) return false;
    // (across ranks: this rank runs the calls on its panel and brings the maxima of its own columns to the one reduction)
    PSMatrix Temp;
    ps_copy(W, RK2);
    ps_increment(K0, RK2, step * 0.5, threshold);
    ps_increment(K1, RK2, step * 0.5, threshold);
    ps_copy(RK1, Temp);
    ps_increment(RK2, Temp, -1.0, threshold);
    m[0] = norm_local(Temp);
    ps_copy(RK2, Temp);
    ps_increment(W, Temp, -1.0, threshold);
    m[1] = norm_local(Temp);
  }
  comm_allreduce_max(m, 2);
  *err = m[0];
  *err2 = m[1];
  return true;
}
bool ps_wom_heun_step(const PSMatrix& W, const PSMatrix& K0, const PSMatrix& K1, const PSMatrix& RK1, double step, double threshold,
                      PSMatrix& RK2out, double* err, double* err2) {
  CommScope cs(W.grid);
  if (!wom_gates({&W, &K0, &K1, &RK1}, &RK2out)) return false;
  DevMat o;
  double m[2] = {0.0, 0.0};
  if (!wom_heun_local(W, K0, K1, RK1, step, threshold, o, m)) return false;
  pack(o);
  install_like(RK2out, W, false, std::move(o));
  comm_allreduce_max(m, 2);
  *err = m[0];
  *err2 = m[1];
  return true;
}
bool ps_wom_c_dots(const PSMatrix& X, const PSMatrix& W, const PSMatrix& XA, double out[2]) {
  CommScope cs(X.grid);
  if (!wom_gates({&X, &W, &XA})) return false;
  double s[2] = {0.0, 0.0};
  const bool taken = slab_on() && slab_enter(mut(X)) && slab_enter(mut(W)) && slab_enter(mut(XA)) && slab_wom_c_dots(X.loc, W.loc, XA.loc, s);
  if (taken) {
    g_slab_counts[2] += 2;   // the two dots
    wom_session_counts()[2] += 1;
  } else {
    wom_session_counts()[3] += 1;
    if (!world().active()) return false;
    double d[2];
    dot_local(X, W, d);
    s[0] = d[0];
    dot_local(W, XA, d);
    s[1] = d[0];
  }
  comm_allreduce_sum(s, 2);
  out[0] = s[0];
  out[1] = s[1];
  return true;
}

long long* purify_session_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// the gates of a fused extrapolator tail that are the same on every rank: a call they keep out is neither fused nor refused, and
// past them every rank enters the same two reductions
bool purify_gates(std::initializer_list<const PSMatrix*> ms, const PSMatrix* out = nullptr) {
  if (options().purify_session < 2 || g_slab_depth == 0 || !all_distinct(ms) || !same_dim(ms) || blk_any(ms)) return false;
  for (const PSMatrix* m : ms)
    if (m->cplx || m->loc.blocked() || labelled(*m) || m == out) return false;
  return world().active() || slab_on();
}
// the tail on this rank's panel: `out` = N' in the fold branch, parts = {dot, 0, norm} of the panel; false: refused (counted)
bool purify_tail_local(const PSMatrix& D, const PSMatrix& N, const PSMatrix& S, bool fold, DevMat& out, double parts[3]) {
  const bool taken = slab_on() && slab_enter(mut(S)) && slab_enter(mut(D)) && slab_enter(mut(N)) &&
                     slab_purify_tail(D.loc, N.loc, S.loc, fold, out, &parts[2], parts);
  if (taken) {
    g_slab_counts[1] += fold ? 3 : 2;   // the merges and the copy
    g_slab_counts[2] += fold ? 3 : 2;   // (the scaling,) the norm and the dot
    purify_session_counts()[fold ? 1 : 2] += 1;
  } else {
    purify_session_counts()[3] += 1;
  }
  return taken;
}
}  // namespace
bool ps_purify_tail(const PSMatrix& D, PSMatrix& N, const PSMatrix& S, bool fold, double* norm, double* next_trace) {
  CommScope cs(D.grid);
  if (!purify_gates({&D, &N, &S})) return false;
  DevMat o;
  double s[3] = {0.0, 0.0, 0.0};
  if (purify_tail_local(D, N, S, fold, o, s)) {
    if (fold) install_like(N, D, false, std::move(o));
  } else {
    if (!world().active()) return false;
    // (across ranks: this rank runs the calls on its panel and brings its parts to the two reductions)
    if (fold) {
      ps_scale(N, -1.0);
      ps_increment(D, N, 2.0, 0.0);
    }
    PSMatrix Temp;
    ps_copy(D, Temp);
    ps_increment(N, Temp, -1.0, 0.0);
    s[2] = norm_local(Temp);
    dot_local(N, S, s);
  }
  comm_allreduce_sum(s, 2);
  comm_allreduce_max(&s[2], 1);
  *next_trace = s[0];
  *norm = s[2];
  return true;
}
bool ps_purify_tail_step(const PSMatrix& D, const PSMatrix& N, const PSMatrix& S, bool fold, PSMatrix& Nout, double* norm, double* next_trace) {
  CommScope cs(D.grid);
  // (one rank only: a refusal is this rank's own answer, so across ranks the call is gated before any rank could wait in a reduction)
  if (world().active() || !purify_gates({&D, &N, &S}, &Nout)) return false;
  DevMat o;
  double s[3] = {0.0, 0.0, 0.0};
  if (!purify_tail_local(D, N, S, fold, o, s)) return false;
  if (fold) pack(o);
  else o = packed_copy(N.loc);
  install_like(Nout, D, false, std::move(o));
  *next_trace = s[0];
  *norm = s[2];
  return true;
}

long long* pade_session_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// the chain on this rank's panels into o1 / o2; false: kept out by a gate (counted nowhere) or refused (counted).  No reduction is
// entered and the calls it replaces are local, so across ranks a refusal is the rank's own
bool pade_chain_local(const PSMatrix& Base, const PSMatrix* const* A, int n_addends, const double scales[2], const double* coeffs,
                      const PSMatrix* out1, const PSMatrix* out2, DevMat& o1, DevMat& o2) {
  if (options().pade_session < 2 || g_slab_depth == 0 || (n_addends != 1 && n_addends != 3) || out1 == out2) return false;
  const PSMatrix* ms[4] = {&Base, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_addends; ++k) ms[k + 1] = A[k];
  for (int k = 0; k <= n_addends; ++k) {
    const PSMatrix* m = ms[k];
    if (!m || m->cplx || m->dim != Base.dim || m->loc.blocked() || labelled(*m) || m == out1 || m == out2) return false;
    for (int i = 0; i < k; ++i)
      if (ms[i] == m) return false;
  }
  bool taken = slab_on();
  const DevMat* locs[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; taken && k <= n_addends; ++k) taken = slab_enter(mut(*ms[k]));
  for (int k = 0; k < n_addends; ++k) locs[k] = &A[k]->loc;
  taken = taken && slab_pade_chain(Base.loc, locs, n_addends, scales, coeffs, o1, o2);
  if (taken) {
    g_slab_counts[1] += 2 * (n_addends + 1);                                      // the copies and the merges
    g_slab_counts[2] += (scales[0] != 1.0 ? 1 : 0) + (scales[1] != 1.0 ? 1 : 0);   // the scalings
    pade_session_counts()[n_addends == 3 ? 1 : 2] += 1;
  } else {
    pade_session_counts()[3] += 1;
  }
  return taken;
}
}  // namespace
bool ps_pade_chain(const PSMatrix& Base, const PSMatrix* const* addends, int n_addends, const double scales[2], const double* coeffs,
                   PSMatrix& Out1, PSMatrix& Out2) {
  CommScope cs(Base.grid);
  DevMat o1, o2;
  if (!pade_chain_local(Base, addends, n_addends, scales, coeffs, &Out1, &Out2, o1, o2)) return false;
  install_like(Out1, Base, false, std::move(o1));
  install_like(Out2, Base, false, std::move(o2));
  return true;
}
bool ps_pade_chain_step(const PSMatrix& Base, const PSMatrix* const* addends, int n_addends, const double scales[2], const double* coeffs,
                        PSMatrix& Out1, PSMatrix& Out2) {
  CommScope cs(Base.grid);
  DevMat o1, o2;
  if (world().active() || !pade_chain_local(Base, addends, n_addends, scales, coeffs, &Out1, &Out2, o1, o2)) return false;
  pack(o1);
  pack(o2);
  install_like(Out1, Base, false, std::move(o1));
  install_like(Out2, Base, false, std::move(o2));
  return true;
}

long long* poly_step_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
namespace {
// the step's tail on this rank's panels into t / r; out1 / out2: the handles the results go to where they are not the step's own
// (the diagnostic).  false: kept out by a gate (counted nowhere) or refused (counted).  No reduction is entered and the calls it
// replaces are local, so across ranks a refusal is the rank's own
bool poly_step_local(const PSMatrix& P, const PSMatrix& Tkm2, const PSMatrix& R, double a, double c, const PSMatrix* out1, const PSMatrix* out2,
                     DevMat& t, DevMat& r) {
  if (options().poly_step < 2 || !slab_on() || (P.grid && P.grid->num_slices > 1)) return false;
  const PSMatrix* ms[3] = {&P, &Tkm2, &R};
  for (const PSMatrix* m : ms)
    if (m->cplx || m->dim != P.dim || m->loc.blocked() || labelled(*m) || m == out1 || m == out2) return false;
  if (&P == &Tkm2 || &P == &R || &Tkm2 == &R || a == 0.0 || c == 0.0) return false;
  const bool taken = slab_enter(mut(P)) && slab_enter(mut(Tkm2)) && slab_enter(mut(R)) && slab_poly_step(P.loc, Tkm2.loc, R.loc, a, c, t, r);
  if (taken) {
    g_slab_counts[1] += 2;   // the two merges
    poly_step_counts()[1] += 1;
  } else {
    poly_step_counts()[2] += 1;
  }
  return taken;
}
}  // namespace
bool ps_poly_step(const PSMatrix& P, const PSMatrix& Tkm2, PSMatrix& Tk, PSMatrix& R, double a, double c) {
  CommScope cs(P.grid);
  if (&Tk == &R || &Tk == &Tkm2) return false;
  DevMat t, r;
  if (!poly_step_local(P, Tkm2, R, a, c, nullptr, nullptr, t, r)) return false;
  install_like(Tk, P, false, std::move(t));
  install_like(R, P, false, std::move(r));
  return true;
}
bool ps_poly_step_diag(const PSMatrix& P, const PSMatrix& Tkm2, const PSMatrix& R, double a, double c, PSMatrix& TkOut, PSMatrix& ROut) {
  CommScope cs(P.grid);
  DevMat t, r;
  if (world().active() || &TkOut == &ROut || !poly_step_local(P, Tkm2, R, a, c, &TkOut, &ROut, t, r)) return false;
  pack(t);
  pack(r);
  install_like(TkOut, P, false, std::move(t));
  install_like(ROut, P, false, std::move(r));
  return true;
}

long long* sum_chain_counts() {
  static long long counts[2] = {0, 0};
  return counts;
}
long long* complex_sum_chain_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}
namespace {
// the chain on this rank's panels into o; out: the handle the result goes to (Base, or none of the inputs).  false: kept out by a
// gate (counted nowhere) or refused (counted).  No reduction is entered and the calls it replaces are local, so across ranks a
// refusal is the rank's own.  Real operands: option sum_chain, counted in sum_chain_counts(); ALL operands complex: option
// complex_sum_chain = 2 inside a session that takes complex operands, counted in complex_sum_chain_counts() only (no view enters:
// a stored (0, 0) refuses); real and complex operands mixed are a gate
bool sum_chain_local(const PSMatrix& Base, double s, const PSMatrix* const* A, const double* coeffs, int n_addends, double post, const PSMatrix* out,
                     DevMat& o) {
  const bool cplx = Base.cplx;
  if (cplx ? (options().complex_sum_chain < 2 || !session_takes(true)) : options().sum_chain == 0) return false;
  if (!slab_on() || n_addends < 1 || n_addends > 5 || (Base.grid && Base.grid->num_slices > 1)) return false;
  long long* counts = cplx ? complex_sum_chain_counts() + 1 : sum_chain_counts();   // ([0] fused, [1] refused)
  const PSMatrix* ms[6] = {&Base, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_addends; ++k) ms[k + 1] = A[k];
  for (int k = 0; k <= n_addends; ++k) {
    const PSMatrix* m = ms[k];
    if (!m || m->cplx != cplx || m->dim != Base.dim || m->loc.blocked() || labelled(*m) || (k > 0 && m == out)) return false;
    for (int i = 0; i < k; ++i)
      if (ms[i] == m) return false;
  }
  // (ScaleMatrix by zero and a zero coefficient leave stored zeros)
  if (!std::isfinite(s) || s == 0.0 || !std::isfinite(post) || post == 0.0) return false;
  for (int k = 0; k < n_addends; ++k)
    if (!std::isfinite(coeffs[k]) || coeffs[k] == 0.0) return false;
  bool taken = true;
  const DevMat* locs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool entered[6] = {false, false, false, false, false, false};
  for (int k = 0; taken && k <= n_addends; ++k) {
    entered[k] = !ms[k]->loc.expanded();
    taken = cplx ? slab_enter_c(mut(*ms[k]), nullptr, false) : slab_enter(mut(*ms[k]));
    if (!taken) {
      if (std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
        std::fprintf(stderr, "[sum chain] operand %d of %d does not enter slab form (loose %d, hint %d, %lld entries)\n", k, n_addends,
                     (int)ms[k]->loc.loose(), (int)ms[k]->loc.slab_hint, (long long)ms[k]->loc.nnz);
      // (an operand the slab form cannot hold: the calls the caller now makes must find the others as the option at 0 would --
      // the ones this attempt turned into slab form go back to compressed columns)
      for (int i = 0; i < k; ++i)
        if (entered[i]) pack(mut(*ms[i]));
    }
  }
  for (int k = 0; k < n_addends; ++k) locs[k] = &A[k]->loc;
  taken = taken && slab_sum_chain(Base.loc, s, locs, coeffs, n_addends, post, o);
  if (taken) {
    g_slab_counts[1] += (out != &Base ? 1 : 0) + n_addends;           // the copy and the merges
    g_slab_counts[2] += (s != 1.0 ? 1 : 0) + (post != 1.0 ? 1 : 0);   // the scalings
    counts[0] += 1;
  } else {
    counts[1] += 1;
  }
  return taken;
}
}  // namespace
bool ps_sum_chain(const PSMatrix& Base, double s, const PSMatrix* const* addends, const double* coeffs, int n_addends, double post, PSMatrix& Out) {
  CommScope cs(Base.grid);
  DevMat o;
  if (!sum_chain_local(Base, s, addends, coeffs, n_addends, post, &Out, o)) return false;
  install_like(Out, Base, Base.cplx, std::move(o));
  return true;
}
bool ps_sum_chain_step(const PSMatrix& Base, double s, const PSMatrix* const* addends, const double* coeffs, int n_addends, double post, PSMatrix& Out) {
  CommScope cs(Base.grid);
  DevMat o;
  if (world().active() || !sum_chain_local(Base, s, addends, coeffs, n_addends, post, &Out, o)) return false;
  pack(o);
  install_like(Out, Base, Base.cplx, std::move(o));
  return true;
}

double ps_sigma(const PSMatrix& A) {
  CommScope cs(A.grid);  // MatrixSigma (distributed_algebra_includes/MatrixSigma.f90)
  const double n = ps_norm(A);
  return 1.0 / (n * n);
}

void ps_gershgorin(const PSMatrix& A, double* e_min, double* e_max) {
  CommScope cs(A.grid);  // GershgorinBounds.f90:1-41
  unblock({&A});
  double mn, mx;
  if (slab_on() && A.loc.expanded()) {
    if (slab_gershgorin(A.loc, A.c0, &mn, &mx)) {
      g_slab_counts[2] += 1;
      comm_allreduce_min(&mn, 1);
      comm_allreduce_max(&mx, 1);
      *e_min = mn;
      *e_max = mx;
      return;
    }
    slab_refused({&A});
  } else {
    slab_pack_if({&A});
  }
  gershgorin(A.loc, A.c0, &mn, &mx);
  comm_allreduce_min(&mn, 1);
  comm_allreduce_max(&mx, 1);
  *e_min = mn;
  *e_max = mx;
}

long long* slab_transpose_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// the gates of the slab transpose (option slab_transpose): one rank without process slices, an open session that takes the
// operand's kind, and an operand the pass reads (slab_transpose_operand: no view, no labelled form).  What they keep out takes
// the path on compressed columns and counts nowhere
bool slab_transpose_on(const PSMatrix& A) {
  return options().slab_transpose >= 1 && !world().active() && !(A.grid && A.grid->num_slices > 1) && slab_on() && A.loc.expanded() &&
         session_takes(A.cplx) && slab_transpose_operand(A.loc);
}
}  // namespace

void ps_transpose(const PSMatrix& A, PSMatrix& AT) {
  CommScope cs(A.grid);  // TransposeMatrix_ps
  unblock({&A});
  DevMat R;
  if (world().active()) {
    DevMat full = ps_gather_full(A);
    R = transpose_slice(full, A.c0, A.c1);
  } else if (slab_transpose_on(A)) {
    if (slab_transpose_any(A.loc, false, R)) {
      g_slab_counts[2] += 1;
      slab_transpose_counts()[0] += 1;
    } else {
      // (the transposed extents lie far apart: a refusal in the session's books, but A keeps its slab form -- this one transpose
      // runs on a packed copy and its result stays in compressed columns)
      g_slab_refusals += 1;
      g_slab_counts[3] += 1;
      slab_transpose_counts()[2] += 1;
      if (g_slab_refusals > 4) g_slab_failed = true;
      if (std::getenv("NTPOLY_AMD_DEBUG_SPGEMM"))
        std::fprintf(stderr, "[slab session] a transpose was refused: this one on compressed columns (%d refusals so far)\n", g_slab_refusals);
      DevMat tmp;
      R = transpose(columns_of(A, tmp));
    }
  } else {
    DevMat tmp;
    R = transpose(columns_of(A, tmp));
  }
  install(AT, A.grid, A.dim, A.cplx, A.c0, A.c1, std::move(R));
}

void ps_conjugate(PSMatrix& A) {
  CommScope cs(A.grid);
  if (options().slab_transpose >= 1 && A.cplx && slab_on() && session_takes(true) && A.loc.expanded() && !world().active() &&
      slab_conjugate_c(A.loc)) {
    g_slab_counts[2] += 1;
    slab_transpose_counts()[1] += 1;
    return;
  }
  conjugate(A.loc);
}

bool ps_slab_transpose_step(const PSMatrix& A, PSMatrix& AT, bool conj) {
  CommScope cs(A.grid);
  if (world().active() || (A.grid && A.grid->num_slices > 1)) return false;
  const bool complex_ok = A.cplx && options().complex_sessions != 0 && options().spgemm_fma == 1 && options().complex_tile != 0;
  if (A.cplx && !complex_ok) return false;
  SlabSession ses(true, false, complex_ok);
  if (!ses.opened || !session_takes(A.cplx)) return false;
  unblock({&A});
  DevMat R;
  const bool entered = slab_kind(A.cplx).enter(mut(A)) && slab_transpose_operand(A.loc);
  const bool done = entered && slab_transpose_any(A.loc, conj, R);
  if (entered) slab_transpose_counts()[done ? 0 : 2] += 1;
  pack(mut(A));   // (the session ends with this call: A goes back to compressed columns)
  if (!done) return false;
  pack(R);
  install_like(AT, A, A.cplx, std::move(R));
  return true;
}

// ------------------------------------------------------------------ PowerBounds on one vector (option power_vector)
long long* power_vector_counts() {
  static long long counts[3] = {0, 0, 0};
  return counts;
}

bool ps_power_vector_open(const PSMatrix& A, PowerVector& pv) {
  CommScope cs(A.grid);
  if (A.grid && A.grid->num_slices > 1) return false;   // (a gate: counted nowhere)
  pv.n = A.dim;
  pv.cplx = A.cplx;
  pv.multi = world().active();
  // (the rows of A from its compressed columns, whatever form it is kept in: A itself stays as it is)
  bool ok;
  {
    DevMat tmp;
    const DevMat& Ac = columns_of(A, tmp);
    ok = Ac.rows == A.dim && Ac.cols == A.c1 - A.c0 && power_gather_build(Ac, A.c0, pv.G);
  }
  if (pv.multi) {   // (every rank or none)
    int64_t bad = ok ? 0 : 1;
    comm_allreduce_sum_i64(&bad, 1);
    ok = bad == 0;
  }
  if (!ok) {
    pv.G = PowerGather();
    return false;
  }
  const size_t w = A.cplx ? 2 : 1;
  pv.x.alloc((size_t)pv.n * w);
  pv.y.alloc((size_t)pv.n * w);
  pv.part.alloc((size_t)power_vector_blocks(pv.n) * 3);
  pv.out.alloc(4);
  return true;
}

void ps_power_vector_set(PowerVector& pv, const double* host_x) {
  pv.x.upload(host_x, pv.x.n);
  sync_stream();   // (the caller's array is free again)
}

void ps_power_vector_step(PowerVector& pv, double threshold, bool scale, double sums[3]) {
  const bool fma = options().spgemm_fma != 0;
  if (pv.multi) {
    // (a rank's chains run over the k of its own panel; the ranks' partial vectors are summed, then every rank prunes, reduces
    // and scales the full vector identically)
    power_vector_chains(pv.G, pv.x.p, pv.y.p, threshold, fma, false, pv.part.p);
    world().tr->allreduce(pv.y.p, pv.y.n, true, 0);
    power_vector_tail(pv.n, pv.cplx, pv.x.p, pv.y.p, threshold, pv.part.p);
  } else {
    power_vector_chains(pv.G, pv.x.p, pv.y.p, threshold, fma, true, pv.part.p);
  }
  power_vector_finish(pv.n, pv.part.p, pv.out.p);
  if (scale) power_vector_scale(pv.n, pv.cplx, pv.y.p, pv.out.p, pv.x.p);
  pv.out.download(sums, 3);   // (the step's one read-back)
}

bool ps_power_vector_diag(const PSMatrix& A, const double* x, double* y, double threshold, double sums[3]) {
  CommScope cs(A.grid);
  PowerVector pv;
  if (!ps_power_vector_open(A, pv)) return false;
  ps_power_vector_set(pv, x);
  ps_power_vector_step(pv, threshold, false, sums);
  pv.y.download(y, pv.y.n);
  return true;
}

// ------------------------------------------------------------------ the traces of CGSolver from column dot passes (option cg_dots)
long long* cg_dots_counts() {
  static long long counts[4] = {0, 0, 0, 0};
  return counts;
}
namespace {
// the gates, the same on every rank: a call they keep out is neither done nor refused
bool cg_dots_gates(std::initializer_list<const PSMatrix*> ms) {
  const PSMatrix& U = **ms.begin();
  const int opt = options().cg_dots;
  if (opt == 0 || g_slab_depth == 0 || !session_takes(U.cplx) || (U.grid && U.grid->num_slices > 1)) return false;
  if (U.cplx && (opt < 2 || world().active())) return false;
  for (const PSMatrix* m : ms)
    if (m->cplx != U.cplx || m->dim != U.dim || m->loc.blocked()) return false;
  return world().active() || slab_on();
}
// this rank's sums: the kernel on the operands' slab forms (true), or the same chains on its compressed columns (false)
bool cg_dots_local(const PSMatrix& U1, const PSMatrix& V1, const PSMatrix* U2, const PSMatrix* V2, double threshold, double t[2], double* diag) {
  const bool cplx = U1.cplx;
  auto enter = [cplx](const PSMatrix& M) { return !labelled(M) && (cplx ? slab_enter_c(mut(M)) : slab_enter(mut(M))); };
  if (slab_on() && enter(U1) && enter(V1) && (!U2 || (enter(*U2) && enter(*V2))) &&
      slab_cg_dots(U1.loc, V1.loc, U2 ? &U2->loc : nullptr, V2 ? &V2->loc : nullptr, threshold, t, diag))
    return true;
  {
    DevMat a, b;
    t[0] = cg_dots_columns(columns_of(U1, a), columns_of(V1, b), threshold, diag);
  }
  if (U2) {
    DevMat a, b;
    t[1] = cg_dots_columns(columns_of(*U2, a), columns_of(*V2, b), threshold);
  }
  return false;
}
}  // namespace

bool ps_cg_dots(const PSMatrix& U1, const PSMatrix& V1, const PSMatrix* U2, const PSMatrix* V2, double threshold, double out[2]) {
  CommScope cs(U1.grid);
  if ((U2 == nullptr) != (V2 == nullptr)) return false;
  if (U2 ? !cg_dots_gates({&U1, &V1, U2, V2}) : !cg_dots_gates({&U1, &V1})) return false;
  const int pairs = U2 ? 2 : 1;
  double t[2] = {0.0, 0.0};
  if (cg_dots_local(U1, V1, U2, V2, threshold, t, nullptr)) {
    g_slab_counts[0] += pairs;       // the products
    g_slab_counts[2] += 2 * pairs;   // their transposes and traces
    cg_dots_counts()[1] += 1;
    cg_dots_counts()[3] += 2 * pairs;
  } else {
    cg_dots_counts()[2] += 1;
  }
  comm_allreduce_sum(t, 2);   // (MatrixTrace's reduction, both sums in one)
  out[0] = t[0];
  if (U2) out[1] = t[1];
  return true;
}

bool ps_cg_dots_diag(const PSMatrix& U, const PSMatrix& V, double threshold, double* diag, double* trace) {
  CommScope cs(U.grid);
  const bool complex_ok = U.cplx && complex_slab_loop(U);
  if (U.cplx && !complex_ok) return false;
  SlabSession ses(true, false, complex_ok);
  if (!ses.opened || !cg_dots_gates({&U, &V})) return false;
  std::vector<double> d((size_t)std::max(0, U.c1 - U.c0), 0.0);
  double t[2] = {0.0, 0.0};
  // (an operand without a slab form -- not run-like, an empty panel --: the chains on its compressed columns, as in the loop)
  cg_dots_local(U, V, nullptr, nullptr, threshold, t, d.data());
  comm_allreduce_sum(t, 2);
  // (the session ends with this call: the operands go back to compressed columns)
  if (U.loc.expanded()) pack(mut(U));
  if (V.loc.expanded()) pack(mut(V));
  std::copy(d.begin(), d.end(), diag);
  *trace = t[0];
  return true;
}

bool ps_is_identity(const PSMatrix& A) {
  CommScope cs(A.grid);  // distributed_includes/IsIdentity.f90:7-38
  int64_t d = identity_check(A.loc, A.c0);
  int64_t v[2] = {d < 0 ? 1 : 0, d < 0 ? 0 : d};
  comm_allreduce_sum_i64(v, 2);
  return v[0] == 0 && v[1] == A.dim;
}

double ps_measure_asymmetry(const PSMatrix& A) {
  CommScope cs(A.grid);  // MeasureAsymmetry: norm(A - A^H)
  PSMatrix T;
  ps_transpose(A, T);
  ps_conjugate(T);
  ps_increment(A, T, -1.0, 0.0);
  return ps_norm(T);
}

void ps_symmetrize(PSMatrix& A) {
  CommScope cs(A.grid);  // SymmetrizeMatrix: A <- (A + A^H)/2
  PSMatrix T;
  ps_transpose(A, T);
  ps_conjugate(T);
  ps_increment(T, A, 1.0, 0.0);
  ps_scale(A, 0.5);
}

void ps_similarity(const PSMatrix& A, const PSMatrix& P, const PSMatrix& PInv, PSMatrix& Res, double threshold) {
  CommScope cs(A.grid);
  // SimilarityTransform (PSMatrixAlgebraModule.F90:603-654)
  if (ps_is_identity(P)) {
    ps_copy(A, Res);
    return;
  }
  PSMatrix Temp, Out;
  ps_multiply(P, A, Temp, 1.0, 0.0, threshold);
  ps_multiply(Temp, PInv, Out, 1.0, 0.0, threshold);
  Res = std::move(Out);
}

// ------------------------------------------------------------------ permutations
void permutation_default(Permutation& p, int n) {
  p.index_lookup.resize((size_t)n);
  p.reverse_index_lookup.resize((size_t)n);
  for (int i = 0; i < n; ++i) p.index_lookup[(size_t)i] = p.reverse_index_lookup[(size_t)i] = i + 1;
}
void permutation_reverse(Permutation& p, int n) {
  p.index_lookup.resize((size_t)n);
  p.reverse_index_lookup.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    p.index_lookup[(size_t)i] = n - i;
    p.reverse_index_lookup[(size_t)i] = i + 1;  // as PermutationModule.F90:66 (only index_lookup is used)
  }
}
void permutation_random(Permutation& p, int n) {
  // Fisher-Yates on the root, broadcast to everybody (PermutationModule.F90:92-107 shares the
  // root's permutation the same way).  The reference draws from the Fortran RNG; any permutation
  // gives the same result matrix up to the threshold.
  permutation_default(p, n);
  static std::mt19937_64 rng(42);
  for (int i = n - 1; i > 0; --i) {
    const int j = (int)(rng() % (uint64_t)(i + 1));
    std::swap(p.index_lookup[(size_t)i], p.index_lookup[(size_t)j]);
  }
  comm_bcast_i32(p.index_lookup.data(), n, 0);
  for (int i = 0; i < n; ++i) p.reverse_index_lookup[(size_t)p.index_lookup[(size_t)i] - 1] = i + 1;
}

// PermuteMatrix / UndoPermuteMatrix (LoadBalancerModule.F90:14-92).  The reference multiplies by two
// permutation matrices; out(i,j) = in(perm(i), perm(j)) is computed here by re-indexing and a device
// sort, with the same result (including the pruning of stored zeros by the threshold-0 products).
void ps_permute(const PSMatrix& in, PSMatrix& out, const Permutation& perm, bool undo) {
  CommScope cs(in.grid);
  const int n = in.dim;
  if ((int)perm.index_lookup.size() != n) NTP_FATAL("permutation size does not match the matrix");
  std::vector<int32_t> map((size_t)n);
  if (!undo) {
    // entry (r, c) moves to (inv[r], inv[c])
    for (int i = 0; i < n; ++i) map[(size_t)perm.index_lookup[(size_t)i] - 1] = i;
  } else {
    for (int i = 0; i < n; ++i) map[(size_t)i] = perm.index_lookup[(size_t)i] - 1;
  }
  DevBuf<int32_t> dmap((size_t)n);
  dmap.upload(map.data(), (size_t)n);
  DevMat R;
  if (world().active()) {
    DevMat full = ps_gather_full(in);
    R = remap_general(full, dmap.p, dmap.p, n, in.c0, in.c1, true);
  } else {
    R = remap_general(in.loc, dmap.p, dmap.p, n, 0, n, true);
  }
  sync_stream();
  install(out, in.grid, n, in.cplx, in.c0, in.c1, std::move(R));   // (by value: out may be in)
}

}  // namespace ntp
