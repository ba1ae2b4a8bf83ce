// Remaining solver families of the reference, all of them callers of the distributed algebra (SpGEMM, increment,
// dot, norm) plus, for the "dense" family, one Hermitian eigendecomposition on the GPU (dense.hip, Jacobi):
//   LinearSolversModule.F90 (CG, Cholesky), AnalysisModule.F90 (pivoted Cholesky, ReduceDimension),
//   ExponentialSolversModule.F90:152-271 (Pade), GeometryOptimizationModule.F90, EigenSolversModule.F90,
//   SingularValueSolversModule.F90, FermiOperatorModule.F90, MatrixConversionModule.F90.
// Control flow, scalar formulas and stopping rules follow the cited lines; the arithmetic is the engine's.
#include <algorithm>
#include <cmath>
#include <functional>

#include "engine.hpp"
#include "kernels.hpp"

namespace ntp {

namespace {
SolverParameters with_monitor(const SolverParameters& p, Monitor& mon) {
  monitor_construct(mon, p.monitor_convergence, p.converge_diff);
  return p;
}
void conj_transpose(const PSMatrix& A, PSMatrix& AT) {
  ps_transpose(A, AT);
  if (AT.cplx) ps_conjugate(AT);
}
}  // namespace

// FilterMatrix (PSMatrixModule.F90:1318-1357): entries with |v| > threshold stay
void ps_filter(PSMatrix& m, double threshold) {
  CommScope cs(m.grid);
  m.loc = filter(m.loc, threshold);
}

// GatherMatrixTripletList: every rank receives every entry (ordered by column, then row)
void ps_gather_triplets(const PSMatrix& m, HostTriplets& t) {
  CommScope cs(m.grid);
  DevMat full = ps_gather_full(m);
  to_triplets(full, 0, t);
}

// ------------------------------------------------------------------ CG (LinearSolversModule.F90:31-171)
// the gate of solver_cg's own slab session (option cg_dots): a caller that holds an outer session open across the solve asks it too
bool solver_cg_opens_session(const PSMatrix& AMat, const PSMatrix& BMat, bool* dots_out, bool* complex_session_out) {
  const bool dots = options().cg_dots != 0 && !(AMat.grid && AMat.grid->num_slices > 1);
  const bool complex_session = dots && options().cg_dots >= 2 && AMat.cplx && BMat.cplx && complex_slab_loop(AMat) && !world().active();
  if (dots_out) *dots_out = dots;
  if (complex_session_out) *complex_session_out = complex_session;
  return dots && ((!AMat.cplx && !BMat.cplx) || complex_session);
}
void solver_cg(const PSMatrix& AMat, PSMatrix& XMat, const PSMatrix& BMat, const SolverParameters& p_in) {
  CommScope cs(AMat.grid);
  Monitor mon;
  const SolverParameters p = with_monitor(p_in, mon);
  if (p.be_verbose) {
    log_header("Linear Solver");
    log_enter();
    log_element("Method", "CG");
    print_parameters(p);
  }
  PSMatrix Identity, ABalanced, BBalanced, RMat, PMat, QMat, RMatT, PMatT, TempMat, X;
  ps_construct_like(Identity, AMat);
  ps_fill_identity(Identity);
  balance_permute(Identity, p);
  balance_copy(AMat, ABalanced, p);
  balance_copy(BMat, BBalanced, p);
  // Option cg_dots: of the iteration's four products three exist only to be traced, and entry (j, j) of U^H V is the dot of column
  // j of U with column j of V -- so the loop runs in a slab session (R, P, Q and X stay in slab form around the one product
  // Q = A P) and takes top, bottom and the new top from column dot passes over the runs (ps_cg_dots: the bits of transpose +
  // product + trace).  1: real operands; 2: also complex ones on one rank in a complex session.  A call the gates keep out runs
  // the three calls as before
  bool dots = false, complex_session = false;
  const bool eligible = solver_cg_opens_session(AMat, BMat, &dots, &complex_session);
  SlabSession slab(eligible, false, complex_session);
  ps_copy(Identity, X);                                                        // initial guess X = I (:89)
  ps_multiply(ABalanced, X, TempMat, 1.0, 0.0, p.threshold);
  ps_copy(BBalanced, RMat);
  ps_increment(TempMat, RMat, -1.0, 0.0);
  ps_copy(RMat, PMat);
  if (p.be_verbose) {
    log_header("Iterations");
    log_enter();
  }
  // trace(prune(U^H V)) the old way
  auto traced_product = [&](const PSMatrix& U, PSMatrix& UT, const PSMatrix& V) {
    conj_transpose(U, UT);
    ps_multiply(UT, V, TempMat, 1.0, 0.0, p.threshold);
    return ps_trace(TempMat);
  };
  double top = 0.0, both[2];
  bool have_top = false, counted = false;   // (have_top: the new top of the last iteration is this one's top -- same matrix, same bits)
  auto count_solve = [&]() {
    if (!counted) cg_dots_counts()[0] += 1;
    counted = true;
  };
  int II;
  for (II = 1; II <= p.max_iterations; ++II) {                                 // :101-139
    ps_multiply(ABalanced, PMat, QMat, 1.0, 0.0, p.threshold);
    double bottom;
    if (dots && (have_top ? ps_cg_dots(PMat, QMat, nullptr, nullptr, p.threshold, both) : ps_cg_dots(PMat, QMat, &RMat, &RMat, p.threshold, both))) {
      count_solve();
      bottom = both[0];
      if (have_top) cg_dots_counts()[3] += 2;   // (the carried top: a product and a transpose more)
      else top = both[1];
    } else {
      if (!have_top) top = traced_product(RMat, RMatT, RMat);
      bottom = traced_product(PMat, PMatT, QMat);
    }
    double step_size = top / bottom;
    ps_increment(PMat, X, step_size, 0.0);
    const double norm_value = std::fabs(step_size * ps_norm(PMat));
    ps_increment(QMat, RMat, -1.0 * step_size, 0.0);
    double new_top;
    if (dots && ps_cg_dots(RMat, RMat, nullptr, nullptr, p.threshold, both)) {
      count_solve();
      new_top = both[0];
    } else {
      new_top = traced_product(RMat, RMatT, RMat);
    }
    step_size = new_top / top;
    ps_scale(PMat, step_size);
    ps_increment(RMat, PMat, 1.0, 0.0);
    top = new_top;
    have_top = dots;
    monitor_append(mon, norm_value);
    if (monitor_converged(mon, p.be_verbose)) break;
  }
  slab.close();
  ps_slab_leave(X);
  if (p.be_verbose) {
    log_exit();
    log_element("Total Iterations", II - 1);
    print_matrix_information(X);
  }
  balance_undo(X, p);
  if (p.be_verbose) log_exit();
  XMat = std::move(X);
}

// ------------------------------------------------------------------ Pade exponential (ExponentialSolversModule.F90:152-271)
void compute_exponential_pade(const PSMatrix& In, PSMatrix& OutMat, const SolverParameters& p) {
  CommScope cs(In.grid);
  if (p.be_verbose) {
    log_header("Exponential Solver");
    log_enter();
    log_element("Method", "Pade");
    print_parameters(p);
  }
  PSMatrix IdentityMat, ScaledMat, TempMat, B1, B2, B3, P1, P2, LeftMat, RightMat, Out;
  ps_construct_like(IdentityMat, In);
  ps_fill_identity(IdentityMat);
  const double spectral_radius = ps_norm(In);
  double sigma_val = 1.0;
  int sigma_counter = 1;
  while (spectral_radius / sigma_val > 1.0) {
    sigma_val *= 2;
    ++sigma_counter;
  }
  ps_copy(In, ScaledMat);
  // the reference divides in default REAL kind: 1.0 / sigma_val with sigma_val a power of two is exact either way
  ps_scale(ScaledMat, 1.0 / sigma_val);
  if (p.be_verbose) {
    log_element("Sigma", sigma_val);
    log_element("Scaling Steps", sigma_counter);
  }
  SolverParameters sub = p;
  sub.threshold = sub.threshold / sigma_val;
  // Option pade_session: everything around the CG solve runs in a slab session as purification_extrapolate's loop does (the powers,
  // both Pade sums, P2, LeftMat and RightMat stay in slab form; real operands, no process slices; the norm above was taken before
  // it opens), 2: each of the two groups of merges is one pass over the runs (ps_pade_chain); a pass that is refused runs the
  // calls.  Where solver_cg opens a session of its own (solver_cg_opens_session) the outer one stays open across it and LeftMat
  // and RightMat enter CG in slab form; otherwise they are packed, the session is closed before the solve -- the CG loop on
  // compressed columns, as cg_dots = 0 promises -- and a second one is opened for the squarings behind it.  The same with a load
  // balancer's permutation: solver_cg permutes its operands BEFORE its session opens, and ps_permute reads compressed columns.
  // solver_cg packs X when its own session closes, so X re-enters once at the first squaring.  A call the gates keep out runs
  // the calls as before
  const bool session = options().pade_session != 0 && !In.cplx && !(In.grid && In.grid->num_slices > 1);
  SlabSession slab(session);
  const bool in_session = slab.opened;
  if (in_session) pade_session_counts()[0] += 1;
  ps_multiply(ScaledMat, ScaledMat, B1, 1.0, 0.0, sub.threshold);
  ps_multiply(B1, B1, B2, 1.0, 0.0, sub.threshold);
  ps_multiply(B2, B2, B3, 1.0, 0.0, sub.threshold);
  // CopyMatrix(Base, Out); ScaleMatrix(Out, s); IncrementMatrix(A, Out, c): in the session one ps_copy_axpby, which has their bits
  auto copy_scale_add = [&](const PSMatrix& Base, double s, const PSMatrix& A, double c, PSMatrix& Res) {
    if (in_session) {
      ps_copy_axpby(Base, A, Res, c, s, 0.0);
      return;
    }
    ps_copy(Base, Res);
    if (s != 1.0) ps_scale(Res, s);
    ps_increment(A, Res, c, 0.0);
  };
  {
    const PSMatrix* powers[3] = {&B1, &B2, &B3};
    const double s[2] = {17297280.0, 8648640.0}, c[6] = {1995840.0, 25200.0, 56.0, 277200.0, 1512.0, 1.0};
    if (!(in_session && ps_pade_chain(IdentityMat, powers, 3, s, c, P1, TempMat))) {
      copy_scale_add(IdentityMat, s[0], B1, c[0], P1);                         // :222-226
      ps_increment(B2, P1, c[1], 0.0);
      ps_increment(B3, P1, c[2], 0.0);
      copy_scale_add(IdentityMat, s[1], B1, c[3], TempMat);                    // :228-234
      ps_increment(B2, TempMat, c[4], 0.0);
      ps_increment(B3, TempMat, c[5], 0.0);
    }
  }
  ps_multiply(ScaledMat, TempMat, P2, 1.0, 0.0, sub.threshold);
  {
    const PSMatrix* addend[1] = {&P2};
    const double s[2] = {1.0, 1.0}, c[2] = {-1.0, 1.0};
    if (!(in_session && ps_pade_chain(P1, addend, 1, s, c, LeftMat, RightMat))) {
      copy_scale_add(P1, 1.0, P2, -1.0, LeftMat);
      copy_scale_add(P1, 1.0, P2, 1.0, RightMat);
    }
  }
  if (in_session && (sub.do_load_balancing || !solver_cg_opens_session(LeftMat, RightMat))) {
    ps_slab_leave(LeftMat);
    ps_slab_leave(RightMat);
    slab.close();
  }
  solver_cg(LeftMat, Out, RightMat, sub);
  SlabSession behind(in_session && !slab.opened);
  const bool squaring_in_session = slab.opened || behind.opened;
  for (int II = 1; II <= sigma_counter - 1; ++II) {                            // undo the scaling by squaring
    ps_multiply(Out, Out, TempMat, 1.0, 0.0, p.threshold);
    if (squaring_in_session) Out = std::move(TempMat);   // (the next squaring rebuilds TempMat before it is read)
    else ps_copy(TempMat, Out);
  }
  if (in_session) {
    behind.close();
    slab.close();
    ps_slab_leave(Out);
  }
  if (p.be_verbose) {
    print_matrix_information(Out);
    log_exit();
  }
  OutMat = std::move(Out);
}

// ------------------------------------------------------------------ GeometryOptimizationModule.F90
void purification_extrapolate(const PSMatrix& PreviousDensity, const PSMatrix& Overlap, double trace, PSMatrix& NewDensityOut,
                              const SolverParameters& p_in) {
  CommScope cs(PreviousDensity.grid);                  // :24-136
  last_trace() = SolverTrace();
  drop_pending_exchange();
  Monitor mon;
  const SolverParameters p = with_monitor(p_in, mon);
  solver_header("Density Matrix Extrapolator", "niklasson2010trace", p, "Purification");
  PSMatrix NewDensity, WorkingDensity, WorkingOverlap, TempMat;
  ps_construct_like(NewDensity, PreviousDensity);
  ps_copy(PreviousDensity, WorkingDensity);
  ps_copy(Overlap, WorkingOverlap);
  balance_permute(WorkingDensity, p);
  balance_permute(WorkingOverlap, p);
  // Option purify_session: the loop runs in a slab session as WOM's does (the density, the overlap and both products stay in slab
  // form; real operands, no process slices; CopyMatrix(NewDensity, WorkingDensity) is a move), 2: everything behind the two
  // products -- the fold, the norm of the change and the NEXT iteration's trace -- is one pass over the runs (ps_purify_tail); a
  // trace the pass did not leave (the first iteration, a refused pass) comes from ps_dot.  A call the gates keep out runs the
  // calls as before
  const bool session = options().purify_session != 0 && !PreviousDensity.cplx && !Overlap.cplx &&
                       !(PreviousDensity.grid && PreviousDensity.grid->num_slices > 1);
  SlabSession slab(session);
  if (slab.opened) purify_session_counts()[0] += 1;
  if (p.be_verbose) {
    log_header("Iterations");
    log_enter();
  }
  double carried_trace = 0.0;
  bool have_trace = false, moved = false;   // (moved: the result sits in WorkingDensity)
  int II;
  for (II = 1; II <= p.max_iterations; ++II) {
    ps_multiply(WorkingDensity, WorkingOverlap, TempMat, 1.0, 0.0, p.threshold);
    ps_multiply(TempMat, WorkingDensity, NewDensity, 1.0, 0.0, p.threshold);
    double trace_value = carried_trace;
    if (!have_trace) {
      double d[2];
      ps_dot(WorkingDensity, WorkingOverlap, d);
      trace_value = d[0];
    }
    const bool fold = trace > trace_value;
    double norm_value = 0.0;
    have_trace = session && ps_purify_tail(WorkingDensity, NewDensity, WorkingOverlap, fold, &norm_value, &carried_trace);
    if (!have_trace) {
      if (fold) {
        ps_scale(NewDensity, -1.0);
        ps_increment(WorkingDensity, NewDensity, 2.0, 0.0);
      }
      ps_increment(NewDensity, WorkingDensity, -1.0, 0.0);
      norm_value = ps_norm(WorkingDensity);
    }
    {
      SolverTrace& t = last_trace();
      t.value.push_back(norm_value);
      t.sigma.push_back(fold ? 1.0 : -1.0);
      t.energy.push_back(trace_value);
      t.nnz.push_back(NewDensity.loc.nnz);
      t.iterations += 1;
    }
    if (slab.opened) {   // (the next iteration rebuilds NewDensity before it is read)
      WorkingDensity = std::move(NewDensity);
      moved = true;
    } else {
      ps_copy(NewDensity, WorkingDensity);
    }
    monitor_append(mon, norm_value);
    if (monitor_converged(mon, p.be_verbose)) break;
    if (p.be_verbose) {
      log_enter();
      log_element("Trace", trace_value);
      log_exit();
    }
  }
  if (moved) NewDensity = std::move(WorkingDensity);   // (the result is in hand wherever the loop ended)
  if (slab.opened) {
    slab.close();
    ps_slab_leave(NewDensity);
  }
  if (p.be_verbose) {
    log_exit();
    log_element("Total Iterations", II);
    print_matrix_information(NewDensity);
  }
  balance_undo(NewDensity, p);
  if (p.be_verbose) log_exit();
  NewDensityOut = std::move(NewDensity);
}

void lowdin_extrapolate(const PSMatrix& PreviousDensity, const PSMatrix& OldOverlap, const PSMatrix& NewOverlap,
                        PSMatrix& NewDensity, const SolverParameters& p) {
  CommScope cs(PreviousDensity.grid);     // :137-214
  solver_header("Density Matrix Extrapolator", "exner2002comparison", p, "Lowdin");
  PSMatrix SQRMat, ISQMat, TempMat, Out;
  solver_square_root(OldOverlap, SQRMat, p, false, 5);
  solver_square_root(NewOverlap, ISQMat, p, true, 5);
  ps_similarity(PreviousDensity, SQRMat, SQRMat, TempMat, p.threshold);
  ps_similarity(TempMat, ISQMat, ISQMat, Out, p.threshold);
  if (p.be_verbose) log_exit();
  NewDensity = std::move(Out);
}

// ------------------------------------------------------------------ MatrixConversionModule.F90:12-43
void snap_to_sparsity_pattern(PSMatrix& mat, const PSMatrix& pattern) {
  CommScope cs(pattern.grid);
  PSMatrix ones, zeros, filtered;
  if (pattern.cplx) ps_to_real(pattern, ones);
  else ps_copy(pattern, ones);
  {  // every stored value of the pattern becomes 1
    const int32_t width = ones.c1 - ones.c0;
    ones.loc = to_real(ones.loc);
    if (ones.loc.nnz) {
      std::vector<double> one((size_t)ones.loc.nnz, 1.0);
      ones.loc.val.upload(one.data(), one.size());
      sync_stream();
    }
    (void)width;
  }
  ps_copy(ones, zeros);
  ps_scale(zeros, 0.0);
  if (mat.cplx) {
    PSMatrix zc, oc;
    ps_to_complex(zeros, zc);
    ps_to_complex(ones, oc);
    zeros = std::move(zc);
    ones = std::move(oc);
  }
  ps_increment(zeros, mat, 1.0, -1.0);   // union pattern, explicit zeros kept (threshold -1)
  ps_copy(mat, filtered);
  ps_pairwise(ones, filtered, mat);
}

// ------------------------------------------------------------------ eigendecomposition (EigenSolversModule.F90:33-71,
// eigenexa_includes/EigenSerial.f90): gather, dense Hermitian eigensolver (dense.hip), drop the pairs past nvals, sparsify with
// the threshold, hand every rank its panel.  Every rank factors the gathered matrix itself (same input, same
// code, same device type), so no broadcast of the vectors is needed.
void ps_eigendecomposition(const PSMatrix& A, PSMatrix& eigenvalues, PSMatrix* eigenvectors, int nvals,
                           const SolverParameters& p) {
  CommScope cs(A.grid);
  if (p.be_verbose) {
    log_header("Eigen Solver");
    log_enter();
    log_element("Method", "Jacobi");
    log_element("NVALS", nvals);
    log_exit();
    print_parameters(p);
  }
  const int32_t n = A.dim;
  const size_t w = A.cplx ? 2 : 1;
  PSMatrix vals, vecs;
  ps_construct_like(vals, A);
  ps_construct_like(vecs, A);
  std::vector<double> hw((size_t)n);
  {
    DevMat full = ps_gather_full(A);
    DevBuf<double> dense((size_t)n * (size_t)n * w), W((size_t)std::max(n, 1));
    to_dense(full, dense.p, n);
    dense_eigh(dense.p, n, A.cplx, W.p);
    if (nvals < n) dense_zero_columns(dense.p, n, n, std::max(nvals, 0), n, A.cplx);
    if (n) {
      HIP_CHECK(hipMemcpyAsync(hw.data(), W.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream()));
      sync_stream();
    }
    if (eigenvectors) vecs.loc = from_dense(dense.p, n, n, vecs.c0, vecs.c1 - vecs.c0, A.cplx, p.threshold);
    sync_stream();
  }
  HostTriplets t;
  t.cplx = false;
  for (int32_t c = vals.c0; c < vals.c1; ++c) {
    if (c >= nvals || !(std::fabs(hw[(size_t)c]) > p.threshold)) continue;
    t.col.push_back(c + 1);
    t.row.push_back(c + 1);
    t.val.push_back(hw[(size_t)c]);
  }
  vals.cplx = false;  // eigenvalues come back as a real matrix also for complex input (EigenSolversModule.F90:316-318)
  vals.loc = from_triplets(t, n, vals.c1 - vals.c0, vals.c0);
  eigenvalues = std::move(vals);
  if (eigenvectors) *eigenvectors = std::move(vecs);
}

// DenseMatrixFunction (EigenSolversModule.F90:74-131): f(A) = V f(L) V^H
void dense_matrix_function(const PSMatrix& A, PSMatrix& Result, const std::function<double(double)>& func,
                           const SolverParameters& p) {
  CommScope cs(A.grid);
  PSMatrix vecs, vecsT, vals, Out;
  ps_eigendecomposition(A, vals, &vecs, A.dim, p);
  HostTriplets t;
  ps_gather_triplets(vals, t);
  for (size_t i = 0; i < t.size(); ++i) t.val[i] = func(t.val[i]);
  conj_transpose(vecs, vecsT);   // taken BEFORE the scaling (:132-133)
  if (A.cplx) {
    HostTriplets tc;
    tc.cplx = true;
    tc.col = t.col;
    tc.row = t.row;
    tc.val.resize(2 * t.size());
    for (size_t i = 0; i < t.size(); ++i) { tc.val[2 * i] = t.val[i]; tc.val[2 * i + 1] = 0.0; }
    ps_diagonal_scale(vecs, tc);
  } else {
    ps_diagonal_scale(vecs, t);
  }
  ps_multiply(vecs, vecsT, Out, 1.0, 0.0, p.threshold);
  Result = std::move(Out);
}

// SingularValueDecomposition (SingularValueSolversModule.F90:14-52): polar decomposition, then the eigenpairs of H
void ps_svd(const PSMatrix& A, PSMatrix& left, PSMatrix& right, PSMatrix& singular, const SolverParameters& p) {
  CommScope cs(A.grid);
  if (p.be_verbose) {
    log_header("Singular Value Solver");
    log_enter();
    log_element("Method", "Polar");
    print_parameters(p);
  }
  PSMatrix UMat, HMat, L, R, S;
  solver_polar(A, UMat, &HMat, p);
  ps_eigendecomposition(HMat, S, &R, HMat.dim, p);
  ps_multiply(UMat, R, L, 1.0, 0.0, p.threshold);
  if (p.be_verbose) log_exit();
  left = std::move(L);
  right = std::move(R);
  singular = std::move(S);
}

// EstimateGap (EigenSolversModule.F90:153-226)
void estimate_gap(const PSMatrix& H, const PSMatrix& K, double chemical_potential, double* gap, const SolverParameters& p) {
  CommScope cs(H.grid);
  if (p.be_verbose) {
    log_header("Estimate Gap");
    log_enter();
    print_parameters(p);
  }
  PSMatrix KH, ShiftH;
  double e_min, e_max;
  ps_multiply(K, H, KH, 1.0, 0.0, p.threshold);
  if (p.be_verbose) {
    log_header("Estimate Minimum");
    log_enter();
  }
  power_bounds(KH, &e_min, p, false);
  if (p.be_verbose) log_exit();
  if (e_min > 0.0) ps_gershgorin(H, &e_min, &e_max);
  if (p.be_verbose) log_element("Estimated e_min", e_min);
  ps_construct_like(ShiftH, H);
  ps_fill_identity(ShiftH);
  ps_scale(ShiftH, -e_min);
  ps_increment(H, ShiftH, 1.0, 0.0);
  ps_multiply(K, ShiftH, KH, 1.0, 0.0, p.threshold);
  power_bounds(KH, &e_max, p, false);
  e_max = e_max + e_min;
  *gap = 2.0 * (chemical_potential - e_max);
  if (p.be_verbose) {
    log_element("HOMO Estimate", e_max);
    log_element("Gap Estimate", *gap);
    log_exit();
  }
}

// ------------------------------------------------------------------ FermiOperatorModule.F90
namespace {
double foe_erf(double x) {  // :531-546 (its own rational approximation, kept for identical occupations)
  const double a1 = 0.254829592, a2 = -0.284496736, a3 = 1.421413741, a4 = -1.453152027, a5 = 1.061405429, pp = 0.3275911;
  const double z = std::fabs(x);
  const double t = 1.0 / (1.0 + pp * z);
  const double tau = t * (a1 + t * (a2 + t * (a3 + t * (a4 + t * a5))));
  return std::copysign(1.0, x) * (1.0 - tau * std::exp(-z * z));
}
}  // namespace

void compute_dense_foe(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, const double* inv_temp_in,
                       double* energy_out, double* mu_out, const SolverParameters& p) {
  CommScope cs(H.grid);  // :31-248
  const bool do_smearing = inv_temp_in != nullptr;
  const double inv_temp = do_smearing ? *inv_temp_in : 0.0;
  if (p.be_verbose) {
    log_header("Density Matrix Solver");
    log_enter();
    if (do_smearing) {
      log_element("Method", "Dense FOE");
      log_element("Inverse Temperature", inv_temp);
    } else {
      log_element("Method", "Dense Step Function");
    }
    print_parameters(p);
  }
  PSMatrix ISQT, WH, WD, vecs, vecsT, vals, Temp, Out;
  ps_transpose(ISQ, ISQT);
  ps_multiply(ISQ, H, Temp, 1.0, 0.0, p.threshold);
  ps_multiply(Temp, ISQT, WH, 1.0, 0.0, p.threshold);
  ps_eigendecomposition(WH, vals, &vecs, WH.dim, p);
  HostTriplets t;
  ps_gather_triplets(vals, t);
  const int num_eigs = H.dim;
  std::vector<double> eigs((size_t)num_eigs, 0.0), occ;
  for (size_t i = 0; i < t.size() && i < (size_t)num_eigs; ++i) eigs[i] = t.val[i];
  double chemical_potential = 0.0;
  int JJ = 1;
  if (do_smearing) {                                                           // bisection on mu (:115-136)
    occ.resize((size_t)num_eigs);
    double left = *std::min_element(eigs.begin(), eigs.end());
    double right = *std::max_element(eigs.begin(), eigs.end());
    for (JJ = 1; JJ <= 10 * p.max_iterations; ++JJ) {
      chemical_potential = left + (right - left) / 2;
      double sv = 0.0;
      for (int i = 0; i < num_eigs; ++i) {
        const double sval = eigs[(size_t)i] - chemical_potential;
        if (inv_temp * sval > 30) occ[(size_t)i] = 0.5 * (1.0 - foe_erf(inv_temp * sval));
        else occ[(size_t)i] = 1.0 / (1.0 + std::exp(inv_temp * sval));
        sv += occ[(size_t)i];
      }
      if (std::fabs(trace - sv) < 1e-8) break;
      else if (sv > trace) right = chemical_potential;
      else left = chemical_potential;
    }
  } else {                                                                     // :137-143
    const int fl = (int)std::floor(trace);
    const double homo = eigs[(size_t)std::max(fl - 1, 0)];
    const double lumo = eigs[(size_t)std::min(fl, num_eigs - 1)];
    const double occ_temp = fl + 1 - trace;
    chemical_potential = homo + occ_temp * 0.5 * (lumo - homo);
  }
  if (p.be_verbose) {
    log_header("Chemical Potential Search");
    log_enter();
    log_element("Potential", chemical_potential);
    log_element("Iterations", JJ);
    log_exit();
  }
  double energy_value = 0.0;                                                   // occupations -> sqrt factors (:153-180)
  for (size_t i = 0; i < t.size(); ++i) {
    if (!do_smearing) {
      if (t.col[i] <= (int)std::floor(trace)) {
        energy_value += t.val[i];
        t.val[i] = 1.0;
      } else if (t.col[i] == (int)std::ceil(trace)) {
        const double occ_temp = trace - std::floor(trace);
        energy_value += occ_temp * t.val[i];
        t.val[i] = std::sqrt(occ_temp);
      } else {
        t.val[i] = 0.0;
      }
    } else {
      const double sval = t.val[i] - chemical_potential;
      const double occ_temp = 1.0 / (1.0 + std::exp(inv_temp * sval));
      energy_value += occ_temp * t.val[i];
      t.val[i] = occ_temp < 0 ? 0.0 : std::sqrt(occ_temp);
    }
  }
  if (vecs.cplx) {
    HostTriplets tc;
    tc.cplx = true;
    tc.col = t.col;
    tc.row = t.row;
    tc.val.resize(2 * t.size());
    for (size_t i = 0; i < t.size(); ++i) { tc.val[2 * i] = t.val[i]; tc.val[2 * i + 1] = 0.0; }
    ps_diagonal_scale(vecs, tc);
  } else {
    ps_diagonal_scale(vecs, t);
  }
  ps_filter(vecs, p.threshold);
  conj_transpose(vecs, vecsT);
  ps_multiply(vecs, vecsT, WD, 1.0, 0.0, p.threshold);
  ps_multiply(ISQT, WD, Temp, 1.0, 0.0, p.threshold);
  ps_multiply(Temp, ISQ, Out, 1.0, 0.0, p.threshold);
  if (energy_out) *energy_out = energy_value;
  if (mu_out) *mu_out = chemical_potential;
  if (p.be_verbose) log_exit();
  K = std::move(Out);
}

namespace {
// ComputeX (:449-473): X = W (I - W^2), optionally hands W^2 back
// (session: option wom_session -- a copy, a scaling and a merge are one ps_copy_axpby where that has their bits)
void wom_compute_x(const PSMatrix& W, const PSMatrix& I, double threshold, PSMatrix& Out, PSMatrix* W2_out, bool session) {
  PSMatrix W2, Temp;
  ps_multiply(W, W, W2, 1.0, 0.0, threshold);
  if (session) {
    ps_copy_axpby(W2, I, Temp, 1.0, -1.0, threshold);   // CopyMatrix(W2, Temp); ScaleMatrix(Temp, -1); IncrementMatrix(I, Temp, 1, threshold)
  } else {
    ps_copy(W2, Temp);
    ps_scale(Temp, -1.0);
    ps_increment(I, Temp, 1.0, threshold);
  }
  ps_multiply(W, Temp, Out, 1.0, 0.0, threshold);
  if (W2_out) *W2_out = std::move(W2);
}
void wom_gc_step(const PSMatrix& X, const PSMatrix& A, double threshold, PSMatrix& Out) {  // :474-483
  ps_multiply(X, A, Out, -0.5, 0.0, threshold);
}
void wom_c_step(const PSMatrix& X, const PSMatrix& A, const PSMatrix& W, double threshold, PSMatrix& Out, bool session) {  // :484-507
  PSMatrix XA;
  ps_multiply(X, A, XA, 1.0, 0.0, threshold);
  double d[2];
  if (!session || !ps_wom_c_dots(X, W, XA, d)) {   // (option wom_session = 2: both dots from one kernel and one read-back)
    double e[2];
    ps_dot(X, W, e);
    d[0] = e[0];
    ps_dot(W, XA, e);
    d[1] = e[0];
  }
  const double denom = d[0], num = d[1];
  if (session) {
    ps_copy_axpby(X, XA, Out, 1.0, -1.0 * num / denom, 0.0);   // CopyMatrix(X, Out); ScaleMatrix(Out, -num / denom); IncrementMatrix(XA, Out)
  } else {
    ps_copy(X, Out);
    ps_scale(Out, -1.0 * num / denom);
    ps_increment(XA, Out, 1.0, 0.0);
  }
  ps_scale(Out, -0.5);
}
}  // namespace

// WOM_Implementation (:317-447): adaptive Heun integration of the wave-operator flow up to inv_temp
void solver_wom(const PSMatrix& H, const PSMatrix& ISQ, PSMatrix& K, double inv_temp, const double* trace_in,
                const double* mu_in, double* energy_out, const SolverParameters& p) {
  CommScope cs(H.grid);
  last_trace() = SolverTrace();
  drop_pending_exchange();
  const bool GC = mu_in != nullptr;
  if (p.be_verbose) {
    log_header("Density Matrix Solver");
    log_enter();
    log_element("Method", GC ? "WOM_GC" : "WOM_C");
    log_element("Inverse Temperature", inv_temp);
    if (GC) log_element("Chemical Potential", *mu_in);
    else log_element("Target Trace", *trace_in);
    print_parameters(p);
  }
  PSMatrix ISQT, WH, IMat, RK1, RK2, K0, K1, Temp, W, A, X, KOrth, Out;
  ps_construct_like(IMat, H);
  ps_fill_identity(IMat);
  ps_transpose(ISQ, ISQT);
  ps_similarity(H, ISQ, ISQT, WH, p.threshold);
  balance_permute(WH, p);
  balance_permute(IMat, p);
  // Option wom_session: the loop runs in a slab session as CGSolver's does (W, A, X, W W, K0, K1, RK1 and RK2 stay in slab form
  // between the six products of a step; real operands, no process slices), 2: the tail of a trial -- RK2, err and err2 -- is one
  // pass over the runs (ps_wom_heun) and the canonical step's two dots are one kernel (ps_wom_c_dots).  A call the gates keep out
  // runs the calls as before
  const bool session = options().wom_session != 0 && !H.cplx && !ISQ.cplx && !(H.grid && H.grid->num_slices > 1);
  SlabSession slab(session);
  if (slab.opened) wom_session_counts()[0] += 1;
  ps_copy(WH, A);
  if (GC) ps_increment(IMat, A, -1.0 * (*mu_in), 0.0);
  ps_copy(IMat, W);
  if (GC) ps_scale(W, 1.0 / std::sqrt(2.0));
  else ps_scale(W, std::sqrt(*trace_in / (double)WH.dim));
  if (p.be_verbose) {
    log_header("Iterations");
    log_enter();
  }
  auto gradient = [&](const PSMatrix& Xm, const PSMatrix& Wm, PSMatrix& Kout) {
    if (GC) wom_gc_step(Xm, A, p.threshold, Kout);
    else wom_c_step(Xm, A, Wm, p.threshold, Kout, session);
  };
  int II = 0;
  double B_I = 0.0, step = 1.0, energy = 0.0;
  while (B_I < inv_temp) {
    step = std::fmin(step, inv_temp - B_I);
    wom_compute_x(W, IMat, p.threshold, X, &KOrth, session);
    double d[2];
    ps_dot(WH, KOrth, d);
    energy = d[0];
    gradient(X, W, K0);
    ++II;
    double err = 0.0, err2 = 0.0;
    bool have_err2 = false;   // (the fused tail computes the accepted step's err2 with every trial's err)
    auto trial = [&]() {                                                       // :358-377 / :380-398
      if (session) {
        ps_copy_axpby(K0, W, RK1, 1.0, step, p.threshold);   // CopyMatrix(K0, RK1); ScaleMatrix(RK1, step); IncrementMatrix(W, RK1, 1, threshold)
      } else {
        ps_copy(K0, RK1);
        ps_scale(RK1, step);
        ps_increment(W, RK1, 1.0, p.threshold);
      }
      wom_compute_x(RK1, IMat, p.threshold, X, nullptr, session);
      gradient(X, RK1, K1);
      ++II;
      have_err2 = session && ps_wom_heun(W, K0, K1, RK1, step, p.threshold, RK2, &err, &err2);
      if (!have_err2) {
        ps_copy(W, RK2);
        ps_increment(K0, RK2, step * 0.5, p.threshold);
        ps_increment(K1, RK2, step * 0.5, p.threshold);
        ps_copy(RK1, Temp);
        ps_increment(RK2, Temp, -1.0, p.threshold);
        err = ps_norm(Temp);
      }
      SolverTrace& t = last_trace();   // (one record per trial, rejected ones included)
      t.value.push_back(err);
      t.sigma.push_back(step);
      t.energy.push_back(energy);
      t.nnz.push_back(RK2.loc.nnz);
      t.iterations += 1;
    };
    trial();
    while (err > 1.1 * p.step_thresh) {
      step = step * std::pow(p.step_thresh / err, 0.5);
      trial();
    }
    if (!have_err2) {
      ps_copy(RK2, Temp);
      ps_increment(W, Temp, -1.0, p.threshold);
      err2 = ps_norm(Temp);
    }
    if (err2 < p.converge_diff) break;                                         // "Early Exit Triggered"
    if (session) W = std::move(RK2);   // (CopyMatrix(RK2, W): the next trial rebuilds RK2 before it is read)
    else ps_copy(RK2, W);
    const double B_I_old = B_I;
    B_I = B_I + step;
    step = step * std::pow(p.step_thresh / err, 0.5);
    if (p.be_verbose) {
      const double sparsity = (double)ps_size(W) / ((double)W.dim * (double)W.dim);
      log_list_element("Gradient Evaluations", (double)II);
      log_enter();
      log_element("Beta", B_I_old);
      log_element("Sparsity", sparsity);
      log_element("Energy", energy);
      log_element("Norm of Change", err2);
      log_exit();
    }
  }
  ps_multiply(W, W, KOrth, 1.0, 0.0, p.threshold);
  if (p.be_verbose) {
    log_exit();
    log_element("Total_Iterations", II);
    print_matrix_information(W);
  }
  if (energy_out) {
    double d[2];
    ps_dot(WH, KOrth, d);
    *energy_out = d[0];
  }
  slab.close();
  ps_slab_leave(KOrth);
  ps_slab_leave(WH);
  balance_undo(KOrth, p);
  ps_similarity(KOrth, ISQT, ISQ, Out, p.threshold);
  if (p.be_verbose) log_exit();
  K = std::move(Out);
}

// ------------------------------------------------------------------ Cholesky (LinearSolversModule.F90:174-300,
// AnalysisModule.F90:26-196).  The reference keeps a dense copy of every rank's block and walks the columns one
// at a time with a broadcast per column; here every rank factors the gathered dense matrix on its GPU and keeps
// its own column panel of L.  rank < 0: plain Cholesky.
void ps_cholesky(const PSMatrix& A, PSMatrix& L, int rank, const SolverParameters& p) {
  CommScope cs(A.grid);
  if (A.cplx) NTP_FATAL("CholeskyDecomposition: real matrices only (as the reference, LinearSolversModule.F90:186-187)");
  if (p.be_verbose) {
    log_header("Linear Solver");
    log_enter();
    if (rank < 0) {
      log_element("Method", "Cholesky Decomposition");
    } else {
      log_element("Method", "Pivoted Cholesky Decomposition");
      log_element("Target_Rank", rank);
      log_citations({"aquilante2006fast"});
    }
    print_parameters(p);
  }
  const int32_t n = A.dim;
  PSMatrix Out;
  ps_construct_like(Out, A);
  {
    DevMat full = ps_gather_full(A);
    DevBuf<double> dA((size_t)n * (size_t)n), dL((size_t)n * (size_t)n);
    to_dense(full, dA.p, n);
    dense_cholesky(dA.p, dL.p, n, p.threshold, rank);
    Out.loc = from_dense(dL.p, n, n, Out.c0, Out.c1 - Out.c0, false, 0.0);
    sync_stream();
  }
  if (p.be_verbose) {
    print_matrix_information(Out);
    log_exit();
  }
  L = std::move(Out);
}

// ReduceDimension (AnalysisModule.F90:199-245)
void reduce_dimension(const PSMatrix& A, int dim, PSMatrix& Reduced, const SolverParameters& p) {
  CommScope cs(A.grid);
  PSMatrix Identity, PMat, PVec, PVecT, VAV;
  ps_construct_like(Identity, A);
  ps_fill_identity(Identity);
  double energy, mu;
  solver_trs4(A, Identity, (double)dim, PMat, &energy, &mu, p);
  ps_cholesky(PMat, PVec, dim, p);
  conj_transpose(PVec, PVecT);
  ps_similarity(A, PVecT, PVec, VAV, p.threshold);
  ps_get_slice(VAV, Reduced, 1, dim, 1, dim);
}

}  // namespace ntp
