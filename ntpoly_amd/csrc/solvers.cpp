// Solver loops of the hot path, driving the device-resident algebra.  Control flow, scalar
// arithmetic and stopping rules follow the reference line by line so that iteration counts match:
//   DensityMatrixSolversModule.F90 (PM :37-281, TRS2 :285-481, TRS4 :485-716, HPCP :720-929)
//   SignSolversModule.F90:150-258, InverseSolversModule.F90:29-149,187-298,
//   SquareRootSolversModule.F90:164-531, ConvergenceMonitorModule.F90, SolverParametersModule.F90,
//   LoggingModule.F90.
// Matrices never leave HBM inside a loop; only scalars (trace, dot, norm, nnz) cross PCIe.
#include <chrono>
#include <cmath>
#include <cstring>

#include "engine.hpp"

namespace ntp {

// ------------------------------------------------------------------ logger
Logger& logger() {
  static Logger* l = new Logger();
  return *l;
}
void log_activate(bool start_document, const char* file_name) {
  Logger& l = logger();
  if (l.owns_file && l.out) std::fclose(l.out);
  l.owns_file = false;
  l.out = stdout;
  if (file_name && file_name[0]) {
    FILE* f = std::fopen(file_name, "w");
    if (!f) NTP_FATAL(std::string("cannot open log file ") + file_name);
    l.out = f;
    l.owns_file = true;
  }
  l.active = true;
  if (start_document) std::fprintf(l.out, "---\n");
}
void log_deactivate() {
  Logger& l = logger();
  if (l.owns_file && l.out) std::fclose(l.out);
  l.owns_file = false;
  l.out = stdout;
  l.active = false;
  l.level = 0;
}
void log_enter() { logger().level += 1; }
void log_exit() { logger().level -= 1; }
static void indent() {
  Logger& l = logger();
  for (int i = 0; i < l.level * 2; ++i) std::fputc(' ', l.out);
}
void log_header(const char* h) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "%s:\n", h);
}
void log_element(const char* key, double v) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "%s: %22.14E\n", key, v);
}
void log_element(const char* key, int v) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "%s: %20d\n", key, v);
}
void log_element(const char* key, const char* v) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "%s: %s\n", key, v);
}
void log_element(const char* key, bool v) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "%s: %s\n", key, v ? "True" : "False");
}
void log_list_element(const char* key, double v) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "- %s: %22.14E\n", key, v);
}
void log_list_element(const char* key) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "- %s\n", key);
}
static void log_list_int(const char* key, long long v) {
  if (!logger().active) return;
  indent();
  std::fprintf(logger().out, "- %s: %10lld\n", key, v);
}

// ------------------------------------------------------------------ monitor
void monitor_construct(Monitor& m, bool automatic, double tight_cutoff) {
  m = Monitor();
  m.automatic = automatic;
  m.tight_cutoff = tight_cutoff;
}
void monitor_append(Monitor& m, double v) {  // ConvergenceMonitorModule.F90:101-119
  for (int i = 0; i < 2; ++i) m.win_short[i] = m.win_short[i + 1];
  for (int i = 0; i < 5; ++i) m.win_long[i] = m.win_long[i + 1];
  m.win_short[2] = v;
  m.win_long[5] = v;
  m.nval += 1;
}
bool monitor_converged(const Monitor& m, bool be_verbose) {  // :122-191
  const double last = m.win_short[2], last2 = m.win_short[1];
  if (be_verbose) log_list_element("Convergence", last);
  bool conv;
  if (std::fabs(last) > m.tight_cutoff) {
    conv = false;
  } else {
    conv = true;
    log_enter();
    log_element("Trigger", "Tight Criteria");
    log_exit();
  }
  if (!m.automatic || conv) return conv;
  conv = true;
  if (m.nval < 6) conv = false;
  double s = 0;
  for (int i = 0; i < 3; ++i) s = s + m.win_short[i];
  const double avg_short = s / 3;
  s = 0;
  for (int i = 0; i < 6; ++i) s = s + m.win_long[i];
  const double avg_long = s / 6;
  if (be_verbose) {
    log_enter();
    log_element("Avg Short", avg_short);
    log_element("Avg Long", avg_long);
    log_exit();
  }
  if (!(10 * avg_short > avg_long && avg_short / 10 < avg_long)) conv = false;
  if (!(10 * last > avg_long && last / 10 < avg_long)) conv = false;
  if (last < 0) conv = false;
  if (std::fabs(last) < std::fabs(last2)) conv = false;
  if (avg_long > m.loose_cutoff) conv = false;
  if (conv) {
    log_enter();
    log_element("Trigger", "Automatic");
    log_exit();
  }
  return conv;
}

void print_parameters(const SolverParameters& p) {  // SolverParametersModule.F90:197-218
  log_header("Solver Parameters");
  log_enter();
  log_element("Verbosity", p.be_verbose);
  log_element("Load Balancing", p.do_load_balancing);
  log_element("Convergence Difference", p.converge_diff);
  log_element("Threshold", p.threshold);
  log_element("Maximum Iterations", p.max_iterations);
  log_element("Step Threshold", p.step_thresh);
  log_element("Monitor Convergence", p.monitor_convergence);
  // (not in the reference's log: which of its two builds the products of this run reproduce -- DESIGN.md section 4.
  // "fma" = the FP-contracted build, every product entry one chain of fma(); "unfused" = the default x86-64 build,
  // separate multiply and add; complex run-like operands in fma mode: two FMA chains per part, a tolerance mode)
  log_element("Arithmetic", options().spgemm_fma == 0 ? "unfused" : "fma");
  log_exit();
}

void print_matrix_information(const PSMatrix& m) {
  CommScope cs(m.grid);  // PSMatrixModule.F90:1248-1266
  double mn = (double)m.loc.nnz, mx = (double)m.loc.nnz;
  comm_allreduce_min(&mn, 1);
  comm_allreduce_max(&mx, 1);
  const double sparsity = (double)ps_size(m) / ((double)m.dim * (double)m.dim);
  log_header("Load_Balance");
  log_enter();
  log_list_int("min_size", (long long)mn);
  log_list_int("max_size", (long long)mx);
  log_exit();
  log_element("Dimension", (int)m.dim);
  log_element("Sparsity", sparsity);
}

SolverTrace& last_trace() {
  static SolverTrace* t = new SolverTrace();
  return *t;
}

// ------------------------------------------------------------------ what the solvers share around their loops
void log_citations(std::initializer_list<const char*> keys) {
  log_header("Citations");
  log_enter();
  for (const char* k : keys) log_list_element(k);
  log_exit();
}
void solver_header(const char* title, const char* citation, const SolverParameters& p, const char* method) {
  if (!p.be_verbose) return;
  log_header(title);
  log_enter();
  if (method) log_element("Method", method);
  log_citations({citation});
  print_parameters(p);
}
void balance_permute(PSMatrix& m, const SolverParameters& p) {
  if (p.do_load_balancing) ps_permute(m, m, p.balance_permutation, false);
}
void balance_copy(const PSMatrix& in, PSMatrix& out, const SolverParameters& p) {
  if (p.do_load_balancing) ps_permute(in, out, p.balance_permutation, false);
  else ps_copy(in, out);
}
void balance_undo(PSMatrix& m, const SolverParameters& p) {
  if (p.do_load_balancing) ps_permute(m, m, p.balance_permutation, true);
}

// "this loop may take complex operands in slab form": FMA arithmetic and the complex tile kernel (sign, inverse, square roots;
// the polynomial and function families of solvers_poly.cpp / solvers_func.cpp under option complex_poly_sessions)
bool complex_slab_loop(const PSMatrix& m) {
  return m.cplx && options().complex_sessions != 0 && options().spgemm_fma == 1 && options().complex_tile != 0;
}

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) {
  sync_stream();
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}
void trace_reset() {   // (every solver's first statement: whatever a panel step of an earlier solve prepared for a successor goes here)
  last_trace() = SolverTrace();
  drop_pending_exchange();
}
// (extra_nnz: entries of the iterate held beside X.loc -- the stored zeros of PM's slab-form iterate)
void trace_rec(double value, double energy, double sigma, const PSMatrix& X, int64_t extra_nnz = 0) {
  SolverTrace& t = last_trace();
  t.value.push_back(value);
  t.energy.push_back(energy);
  t.sigma.push_back(sigma);
  t.nnz.push_back(X.loc.nnz + extra_nnz);
  t.iterations += 1;
}
double real_dot(const PSMatrix& A, const PSMatrix& B) {
  double out[2];
  ps_dot(A, B, out);
  return out[0];
}
void log_iterations_header(const SolverParameters& p) {
  if (!p.be_verbose) return;
  log_header("Iterations");
  log_enter();
}

// What the density solvers share around their loops.  The loop body -- the part that differs, and the part read against
// the Fortran -- stays written out in each solver; so do the communicator scope, the band scope and the slab session,
// which differ per solver.
struct DensityFrame {
  const SolverParameters& p;
  Clock::time_point t0, t1;
  Monitor mon;
  PSMatrix WH, IMat, ISQT;
  double e_min = 0.0, e_max = 0.0;
  double energy_value = 0.0;

  // prologue: header, WH = ISQ H ISQ^T, optional permutation, Gershgorin bounds
  DensityFrame(const char* method, const char* citation, const PSMatrix& H, const PSMatrix& ISQ, const SolverParameters& p_)
      : p(p_) {
    trace_reset();
    t0 = Clock::now();
    monitor_construct(mon, p.monitor_convergence, p.converge_diff);
    solver_header("Density Matrix Solver", citation, p, method);
    ps_construct_like(IMat, H);
    ps_fill_identity(IMat);
    ps_transpose(ISQ, ISQT);
    ps_similarity(H, ISQ, ISQT, WH, p.threshold);
    balance_permute(WH, p);
    balance_permute(IMat, p);
    ps_gershgorin(WH, &e_min, &e_max);
  }
  // X0 = (e_max I - WH) / (e_max - e_min): the spectrum mapped into [0, 1], reversed
  void start_iterate(PSMatrix& X) const {
    ps_copy(WH, X);
    ps_scale(X, -1.0);
    ps_increment(IMat, X, e_max, 0.0);
    ps_scale(X, 1.0 / (e_max - e_min));
  }
  void begin_loop() {
    log_iterations_header(p);
    last_trace().setup_ms = ms_since(t0);
    t1 = Clock::now();
  }
  // tail of one iteration, given the energy of the new iterate X: true when the loop is over
  bool converged(double energy, double sigma, const PSMatrix& X, int64_t extra_nnz = 0) {
    const double energy_old = energy_value;
    energy_value = energy;
    monitor_append(mon, energy_value - energy_old);
    trace_rec(energy_value - energy_old, energy_value, sigma, X, extra_nnz);
    if (monitor_converged(mon, p.be_verbose)) return true;
    if (p.be_verbose) {
      log_enter();
      log_element("Energy Value", energy_value);
      log_exit();
    }
    return false;
  }
  // epilogue, once the iterate X is back in compressed columns: II is the loop counter as the loop left it
  void finish(int II, PSMatrix& X, const PSMatrix& ISQ, PSMatrix& K, double* energy_out) {
    last_trace().loop_ms = ms_since(t1);
    if (p.be_verbose) {
      log_exit();
      log_element("Total Iterations", II);
      print_matrix_information(X);
    }
    if (energy_out) *energy_out = energy_value;
    balance_undo(X, p);
    ps_similarity(X, ISQT, ISQ, K, p.threshold);
    // what the fused / relabelled steps keep for the NEXT solve on the same operand (the expanded WH, WH in the recovered
    // band order: about 8 (nnz + 32 columns) + 12 nnz + 8 n bytes, 1.3 GB at N = 262 144) goes now when the caller said so
    if (!options().operand_cache) drop_operand_caches();
    if (p.be_verbose) log_exit();
  }
};

// The chemical potential from the recorded sigmas: bisection on [0, 1] for the point that the loop's scalar polynomials
// z <- step(z, sigma_JJ), JJ = 1 .. total_iterations, carry to 1/2.  Returns the midpoint; the map back to an energy is the solver's.
template <class Step>
double bisect_mu(const std::vector<double>& sigma_array, int total_iterations, const SolverParameters& p, Step step) {
  double interval_a = 0.0, interval_b = 1.0, midpoint = 0.0;
  for (int it = 1; it <= p.max_iterations; ++it) {
    midpoint = (interval_b - interval_a) / 2.0 + interval_a;
    double z = midpoint;
    for (int JJ = 1; JJ <= total_iterations; ++JJ) z = step(z, sigma_array[(size_t)JJ]);
    if (z < 0.5) interval_a = midpoint;
    else interval_b = midpoint;
    if (std::fabs(z - 0.5) < p.converge_diff) break;
  }
  return midpoint;
}
}  // namespace

// ------------------------------------------------------------------ TRS2
// One iteration of the TRS2 loop (DensityMatrixSolversModule.F90:380-404).  The update
// "ScaleMatrix(X,2); IncrementMatrix(X2,X,-1,threshold); DotMatrix(X,WH)" runs as ONE pass over X, X2
// and WH (same arithmetic: 2*x is exact, then the AddSparseVectors rules, then the energy).
double trs2_step(PSMatrix& X, PSMatrix& X2, const PSMatrix& WH, double trace_target, double threshold, double* sigma,
                 double* trace_io) {
  CommScope cs(WH.grid);
  // trace_io (optional): in = trace(X) if the caller already has it (NaN: compute it), out = trace of the new X,
  // accumulated in the pass that produces the energy -> one reduction + read-back less per iteration
  const double trace_value = (trace_io && *trace_io == *trace_io) ? *trace_io : ps_trace(X);
  *sigma = (trace_target - trace_value < 0.0) ? -1.0 : 1.0;
  double out[4] = {0, 0, 0, 0};
  if (*sigma > 0.0) {
    ps_square_update_dot(X, X2, threshold, WH, out, trace_io != nullptr);  // X = 2X - X*X; energy; trace (X2: scratch -- holds X*X only on the unfused path)
  } else {
    ps_square_dot(X, X2, threshold, WH, out, trace_io != nullptr);         // X = X*X; energy; trace
  }
  if (trace_io) *trace_io = out[2];
  return out[0];
}

void solver_trs2(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy_out, double* mu_out,
                 const SolverParameters& p) {
  CommScope cs(H.grid);
  // (several ranks, an operand without runs: the whole solve in a recovered band order -- band_scope.cpp)
  if (band_scope_try({&H, &ISQ}, {&K}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) {
        solver_trs2(*in[0], *in[1], trace, *out[0], energy_out, mu_out, p);
      }))
    return;
  DensityFrame f("TRS2", "niklasson2002expansion", H, ISQ, p);    // :344-365
  std::vector<double> sigma_array((size_t)p.max_iterations + 1, 0.0);
  PSMatrix X, X2;
  f.start_iterate(X);                                              // :368-371
  f.begin_loop();
  double trace_x = std::nan("");  // trace of the current iterate, handed from step to step
  trs2_complex_reset();
  int II;
  for (II = 1; II <= p.max_iterations; ++II) {                     // :380-413
    static const bool step_times = std::getenv("NTPOLY_AMD_DEBUG_STEPTIME") != nullptr;   // (host clock per iteration, rank 0)
    const auto ts0 = Clock::now();
    const double energy_value = trs2_step(X, X2, f.WH, trace, p.threshold, &sigma_array[(size_t)II], &trace_x);
    const double ts_step = step_times ? ms_since(ts0) : 0.0;   // (ms_since waits for the stream: only when asked for)
    const bool done = f.converged(energy_value, sigma_array[(size_t)II], X);
    if (step_times && world().rank == 0)
      std::fprintf(stderr, "[trs2] iteration %d: step %.3f ms, with the trace record %.3f ms\n", II, ts_step, ms_since(ts0));
    if (done) break;
  }
  const int total_iterations = II - 1;
  pack(X.loc);  // (the steps leave the iterate loose, kernels.hpp)
  f.finish(II, X, ISQ, K, energy_out);                             // :427-434
  if (mu_out) {                                                    // :444-472
    const double midpoint = bisect_mu(sigma_array, total_iterations, p, [](double zero_value, double sg) {
      if (sg < 0.0) zero_value = zero_value * zero_value;
      else zero_value = 2.0 * zero_value - zero_value * zero_value;
      return zero_value;
    });
    *mu_out = f.e_max + (f.e_min - f.e_max) * midpoint;
  }
}

// ------------------------------------------------------------------ TRS4
void solver_trs4(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy_out, double* mu_out,
                 const SolverParameters& p) {
  CommScope cs(H.grid);
  // (several ranks, an operand without runs: the whole solve in a recovered band order -- band_scope.cpp)
  if (band_scope_try({&H, &ISQ}, {&K}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) {
        solver_trs4(*in[0], *in[1], trace, *out[0], energy_out, mu_out, p);
      }))
    return;
  const double sigma_min = 0.0, sigma_max = 6.0;
  DensityFrame f("TRS4", "niklasson2002expansion", H, ISQ, p);
  const PSMatrix &WH = f.WH, &IMat = f.IMat;
  std::vector<double> sigma_array((size_t)p.max_iterations + 1, 0.0);
  PSMatrix X, X2, Fx, Gx, Temp;
  f.start_iterate(X);
  f.begin_loop();
  int II;
  // Option complex_trs4, a complex Hamiltonian on one rank without process slices: a complex session -- the products on the complex
  // tile kernel, the chain below on complex runs (ps_trs4_traces / ps_trs4_operand), the energy from one pass (ps_trs4_energy)
  const bool complex_session = X.cplx && WH.cplx && complex_slab_loop(X) && options().complex_trs4 != 0 && !world().active() &&
                               !(X.grid && X.grid->num_slices > 1);
  SlabSession slab((!X.cplx && !WH.cplx) || complex_session, false, complex_session);   // (the loop's matrices stay in slab form between its operations where they can)
  for (II = 1; II <= p.max_iterations; ++II) {                     // :586-638
    ps_multiply(X, X, X2, 1.0, 0.0, p.threshold);
    // Fx = 4 X - 3 X2, Gx = I - 2 X + X2 and their traces against X2: in a slab session one pass over X and X2 leaves the
    // traces without building Fx and Gx (the same element arithmetic; IMat is the identity also under load balancing)
    double trace_fx = 0.0, trace_gx = 0.0;
    const bool chain_fused = ps_trs4_traces(X, X2, &trace_fx, &trace_gx);
    if (!chain_fused) {
      ps_copy_axpby(X2, X, Fx, 4.0, -3.0, 0.0);                     // CopyMatrix(X2, Fx); ScaleMatrix(Fx, -3); IncrementMatrix(X, Fx, 4)
      ps_copy_axpby(IMat, X, Gx, -2.0, 1.0, 0.0);                   // CopyMatrix(Identity, Gx); IncrementMatrix(X, Gx, -2)
      ps_increment(X2, Gx, 1.0, 0.0);
      trace_fx = real_dot(X2, Fx);
      trace_gx = real_dot(X2, Gx);
    }
    if (std::fabs(trace_gx) < 1.0e-14) sigma_array[(size_t)II] = 0.5 * (sigma_max - sigma_min);
    else sigma_array[(size_t)II] = (trace - trace_fx) / trace_gx;
    if (sigma_array[(size_t)II] > sigma_max) {
      ps_copy_axpby(X, X2, Temp, -1.0, 2.0, 0.0);                   // CopyMatrix(X, Temp); ScaleMatrix(Temp, 2); IncrementMatrix(X2, Temp, -1)
    } else if (sigma_array[(size_t)II] < sigma_min) {
      ps_copy(X2, Temp);
    } else {
      if (!(chain_fused && ps_trs4_operand(X, X2, sigma_array[(size_t)II], Gx))) {
        if (chain_fused) {   // (the traces came from the fused pass but the operand cannot: build the intermediates now)
          ps_copy_axpby(X2, X, Fx, 4.0, -3.0, 0.0);
          ps_copy_axpby(IMat, X, Gx, -2.0, 1.0, 0.0);
          ps_increment(X2, Gx, 1.0, 0.0);
        }
        ps_axpby(Fx, Gx, 1.0, sigma_array[(size_t)II], 0.0);        // ScaleMatrix(Gx, sigma); IncrementMatrix(Fx, Gx)
      }
      ps_multiply(X2, Gx, Temp, 1.0, 0.0, p.threshold);
    }
    // :630-631 IncrementMatrix(TempMat, X_k, -1) is overwritten by the copy that follows it; the copy itself is a
    // hand-over here (Temp is rebuilt in every iteration)
    std::swap(X.loc, Temp.loc);
    double energy_value = 0.0;
    if (!(complex_session && ps_trs4_energy(X, WH, &energy_value))) energy_value = real_dot(X, WH);
    if (f.converged(energy_value, sigma_array[(size_t)II], X)) break;
  }
  const int total_iterations = II - 1;
  slab.close();
  ps_slab_leave(X);
  f.finish(II, X, ISQ, K, energy_out);
  if (mu_out) {                                                    // :669-704
    const double midpoint = bisect_mu(sigma_array, total_iterations, p, [=](double z, double sg) {
      if (sg > sigma_max) z = 2.0 * z - z * z;
      else if (sg < sigma_min) z = z * z;
      else {
        const double tempfx = (z * z) * (4.0 * z - 3.0 * z * z);
        const double tempgx = (z * z) * (1.0 - z) * (1.0 - z);
        z = tempfx + sg * tempgx;
      }
      return z;
    });
    *mu_out = f.e_max + (f.e_min - f.e_max) * midpoint;
  }
}

// ------------------------------------------------------------------ PM
void solver_pm(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy_out, double* mu_out,
               const SolverParameters& p) {
  CommScope cs(H.grid);
  // (several ranks, an operand without runs: the whole solve in a recovered band order -- band_scope.cpp)
  if (band_scope_try({&H, &ISQ}, {&K}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) {
        solver_pm(*in[0], *in[1], trace, *out[0], energy_out, mu_out, p);
      }))
    return;
  DensityFrame f("PM", "palser1998canonical", H, ISQ, p);         // :96-118
  const PSMatrix &WH = f.WH, &IMat = f.IMat;
  const double e_min = f.e_min, e_max = f.e_max;
  std::vector<double> sigma_array((size_t)p.max_iterations + 1, 0.0);
  PSMatrix X, X2, X3, Temp;
  ps_copy(WH, X);
  const double dim = (double)H.dim;
  double trace_value = ps_trace(X);                                // :124-125
  const double lambda = trace_value / dim;
  const double alpha1 = trace / (e_max - lambda);                  // :128-130
  const double alpha2 = (dim - trace) / (lambda - e_min);
  const double alpha = std::fmin(alpha1, alpha2);
  double factor = -alpha / dim;
  ps_scale(X, factor);
  factor = (alpha * lambda + trace) / dim;
  ps_increment(IMat, X, factor, 0.0);
  f.begin_loop();
  int II;
  // Option pm_session, real operands: the loop's matrices stay in slab form, as in TRS4.  Whenever sigma > 1/2 the update scales X
  // by a1 = 0 -- stored zeros whose tails steer the merges that follow, which the runs of a slab form cannot hold: those rows travel
  // in `zeros` beside a zero-free X (slab_extra.hip), the scalars of sigma and the update are one pass each.  Every decision to
  // leave that path is collective and rides on a reduction the iteration makes anyway; it is taken once per solve: the iterate
  // is materialised (compressed columns with the listed rows as stored zeros), the session closed, the loop body below as it was.
  // Option complex_pm, a complex Hamiltonian on one rank without process slices: a complex session, as solver_trs4 opens it -- the
  // products on the complex tile kernel, the same calls on runs of (re, im) pairs with the rows of stored (0, 0) entries in `zeros`.
  // Its books are complex_pm_counts(); a solve whose iterates take block form (a gate, not a refusal) leaves uncounted.
  const bool real = !X.cplx && !WH.cplx;
  const bool complex_session = X.cplx && WH.cplx && complex_slab_loop(X) && options().complex_pm != 0 && !world().active() &&
                               !(X.grid && X.grid->num_slices > 1);
  SlabSession slab((options().pm_session != 0 && real) || complex_session, false, complex_session);
  const bool in_session = slab.opened;
  bool fused = slab.opened;
  ZeroList zeros;
  auto leave_fused = [&](bool counted = true) {
    ps_pm_materialise(X, zeros);
    slab.close();
    ps_slab_leave(X2);
    ps_slab_leave(X3);
    ps_slab_leave(f.WH);
    fused = false;
    if (counted) (complex_session ? complex_pm_counts() : pm_session_counts())[3] += 1;
  };
  for (II = 1; II <= p.max_iterations; ++II) {                     // :145-200
    ps_multiply(X, X, X2, 1.0, 0.0, p.threshold);
    ps_multiply(X, X2, X3, 1.0, 0.0, p.threshold);
    double trace_value2 = 0.0;
    // (an iterate that is no zero-free slab -- the starting iterate stores a zero, a product declined -- is refused here, on every rank)
    bool gated = false;
    if (fused && !ps_pm_sigma(X, zeros, X2, p.threshold, &trace_value, &trace_value2, &gated)) leave_fused(!gated);
    if (!fused) {
      ps_copy(X, Temp);
      ps_increment(X2, Temp, -1.0, p.threshold);
      trace_value = ps_trace(Temp);
      trace_value2 = real_dot(Temp, X);
    }
    if (trace_value <= 2.2250738585072014e-308) sigma_array[(size_t)II] = 1.0;
    else sigma_array[(size_t)II] = trace_value2 / trace_value;
    const double sg = sigma_array[(size_t)II];
    double a1, a2, a3;
    if (sg > 0.5) {
      a1 = 0.0;
      a2 = 1.0 + 1.0 / sg;
      a3 = -1.0 / sg;
    } else {
      a1 = (1.0 - 2.0 * sg) / (1.0 - sg);
      a2 = (1.0 + sg) / (1.0 - sg);
      a3 = -1.0 / (1.0 - sg);
    }
    double energy;
    if (fused) {
      const bool here = ps_pm_update(X, zeros, X2, X3, a1, a2, a3, p.threshold);
      bool some_refused = false;
      energy = ps_pm_energy(X, WH, !here, &some_refused);
      if (some_refused) leave_fused();
    } else {
      ps_axpby(X2, X, a2, a1, p.threshold);                         // ScaleMatrix(X, a1); IncrementMatrix(X2, X, a2)
      ps_increment(X3, X, a3, p.threshold);
      energy = real_dot(X, WH);
    }
    if (f.converged(energy, sg, X, zeros.count)) break;
  }
  if (in_session) {
    slab.close();
    ps_pm_materialise(X, zeros);
  }
  const int total_iterations = II - 1;
  f.finish(II, X, ISQ, K, energy_out);
  if (mu_out) {                                                    // :234-268
    const double midpoint = bisect_mu(sigma_array, total_iterations, p, [](double z, double sg) {
      if (sg > 0.5) {
        z = ((1.0 + sg) * (z * z)) - (z * z * z);
        z = z / sg;
      } else {
        z = ((1.0 - 2.0 * sg) * z) + ((1.0 + sg) * (z * z)) - (z * z * z);
        z = z / (1.0 - sg);
      }
      return z;
    });
    *mu_out = lambda - (dim * midpoint - trace) / alpha;
  }
}

// ------------------------------------------------------------------ HPCP
void solver_hpcp(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double* energy_out, double* mu_out,
                 const SolverParameters& p) {
  CommScope cs(H.grid);
  // (several ranks, an operand without runs: the whole solve in a recovered band order -- band_scope.cpp)
  if (band_scope_try({&H, &ISQ}, {&K}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) {
        solver_hpcp(*in[0], *in[1], trace, *out[0], energy_out, mu_out, p);
      }))
    return;
  DensityFrame f("HPCP", "truflandier2016communication", H, ISQ, p);   // :789-808
  const PSMatrix &WH = f.WH, &IMat = f.IMat;
  const double e_min = f.e_min, e_max = f.e_max;
  std::vector<double> sigma_array((size_t)p.max_iterations + 1, 0.0);
  PSMatrix TempMat, D1, DH, DDH, D2DH;
  const double dim = (double)H.dim;
  double mu = ps_trace(WH) / dim;                                  // :809-817
  const double sigma_bar = (dim - trace) / dim;
  const double sigma = 1.0 - sigma_bar;
  const double beta = sigma / (e_max - mu);
  const double beta_bar = sigma_bar / (mu - e_min);
  const double beta_1 = sigma;
  const double beta_2 = std::fmin(beta, beta_bar);
  ps_copy(IMat, D1);                                               // :820-826
  ps_scale(D1, beta_1);
  ps_copy(IMat, TempMat);
  ps_scale(TempMat, mu);
  ps_increment(WH, TempMat, -1.0, 0.0);
  ps_scale(TempMat, beta_2);
  ps_increment(TempMat, D1, 1.0, 0.0);
  f.begin_loop();
  double trace_value = 0.0;
  int II;
  // Option complex_hpcp, a complex Hamiltonian on one rank without process slices: a complex session, as solver_trs4 opens it -- the
  // products on the complex tile kernel, the two fused calls below on complex runs
  const bool complex_session = D1.cplx && WH.cplx && complex_slab_loop(D1) && options().complex_hpcp != 0 && !world().active() &&
                               !(D1.grid && D1.grid->num_slices > 1);
  SlabSession slab((!D1.cplx && !WH.cplx) || complex_session, false, complex_session);
  // Option hpcp_step, inside the real session: the two traces in one pass behind the second product (ps_hpcp_traces: the bits of
  // the two calls), and the two merges, the energy and the NEXT iteration's DH in one pass over the three runs (ps_hpcp_update).
  // An update that is not taken runs the calls of this iteration, and the next DH is built by the three calls again.
  // (hpcp_step is the real loop's option: complex operands outside a complex session are declined by both calls, as before)
  const bool step = options().hpcp_step != 0 || complex_session;
  bool have_dh = false;   // DH = I - D1 came out of the last update
  for (II = 1; II <= p.max_iterations; ++II) {                     // :836-872
    if (!have_dh) {
      ps_copy(D1, DH);
      ps_increment_identity(IMat, DH, -1.0);                       // IncrementMatrix(Identity, DH, -1)
      ps_scale(DH, -1.0);
    }
    have_dh = false;
    ps_multiply(D1, DH, DDH, 1.0, 0.0, p.threshold);
    double trace_value2;
    if (!step) trace_value = ps_trace(DDH);
    ps_multiply(D1, DDH, D2DH, 1.0, 0.0, p.threshold);
    double both[2];
    if (step && ps_hpcp_traces(DDH, D2DH, both)) {
      trace_value = both[0];
      trace_value2 = both[1];
    } else {
      if (step) trace_value = ps_trace(DDH);
      trace_value2 = ps_trace(D2DH);
    }
    sigma_array[(size_t)II] = trace_value2 / trace_value;
    double energy;
    if (step && ps_hpcp_update(D1, DDH, D2DH, sigma_array[(size_t)II], WH, DH, &energy)) {
      have_dh = true;
    } else {
      ps_increment(D2DH, D1, 2.0, 0.0);
      ps_increment(DDH, D1, -1.0 * 2.0 * sigma_array[(size_t)II], 0.0);
      energy = real_dot(D1, WH);
    }
    if (f.converged(energy, sigma_array[(size_t)II], D1)) break;
  }
  const int total_iterations = II - 1;
  slab.close();
  ps_slab_leave(D1);
  f.finish(II, D1, ISQ, K, energy_out);
  if (mu_out) {                                                    // :896-921
    const double midpoint = bisect_mu(sigma_array, total_iterations, p, [](double z, double sg) {
      return z + 2.0 * (((z * z)) * (1.0 - z) - sg * z * (1.0 - z));
    });
    *mu_out = mu + (beta_1 - midpoint) / beta_2;
  }
}

// ------------------------------------------------------------------ ScaleAndFold
// DensityMatrixSolversModule.F90:953-1117 (rubensson2011nonmonotonic): like TRS2 with the polynomials scaled by the
// running estimates Beta / BetaBar of where lumo and homo have moved to
void solver_scale_and_fold(const PSMatrix& H, const PSMatrix& ISQ, double trace, PSMatrix& K, double homo, double lumo,
                           double* energy_out, const SolverParameters& p) {
  CommScope cs(H.grid);
  DensityFrame f("Scale and Fold", "rubensson2011nonmonotonic", H, ISQ, p);   // :1022-1034
  const PSMatrix &WH = f.WH, &IMat = f.IMat;
  const double e_min = f.e_min, e_max = f.e_max;
  PSMatrix X, X2;
  f.start_iterate(X);                                              // :1036-1039
  double Beta = (e_max - lumo) / (e_max - e_min);
  double BetaBar = (e_max - homo) / (e_max - e_min);
  f.begin_loop();
  int II;
  // Option complex_scale_fold, a complex Hamiltonian on one rank without process slices: a complex session, as solver_trs4 opens it
  // -- the product on the complex tile kernel, the two fused calls below on complex runs
  const bool complex_session = X.cplx && WH.cplx && complex_slab_loop(X) && options().complex_scale_fold != 0 && !world().active() &&
                               !(X.grid && X.grid->num_slices > 1);
  SlabSession slab((!X.cplx && !WH.cplx) || complex_session, false, complex_session);
  // Option scale_fold_step, inside the real session: behind the step's one product the fold branch's update, the energy and the
  // NEXT step's trace are one pass (ps_saf_update), and the scale branch, whose product's result is the new X, takes the energy and
  // the trace from one pass over X and WH (ps_saf_dot_trace).  A step that is not taken runs the calls, and the next step asks for
  // its trace again.
  // (scale_fold_step is the real loop's option: complex operands outside a complex session are declined by both calls, as before)
  const bool step = options().scale_fold_step != 0 || complex_session;
  double trace_x = std::nan("");   // trace(X) as the last fused pass returned it; NaN: not known
  for (II = 1; II <= p.max_iterations; ++II) {                     // :1049-1081
    const double trace_value = std::isnan(trace_x) ? ps_trace(X) : trace_x;
    trace_x = std::nan("");
    double alpha, dot;
    bool fused;
    if (trace_value > trace) {
      alpha = 2.0 / (2.0 - Beta);
      ps_axpby(IMat, X, 1.0 - alpha, alpha, 0.0);                   // ScaleMatrix(X, alpha); IncrementMatrix(I, X, 1 - alpha)
      ps_multiply(X, X, X2, 1.0, 0.0, p.threshold);
      std::swap(X.loc, X2.loc);  // CopyMatrix(X_k2, X_k); X2 is scratch
      fused = step && ps_saf_dot_trace(X, WH, &dot, &trace_x);
      Beta = (alpha * Beta + 1 - alpha) * (alpha * Beta + 1 - alpha);
      BetaBar = (alpha * BetaBar + 1 - alpha) * (alpha * BetaBar + 1 - alpha);
    } else {
      alpha = 2.0 / (1.0 + BetaBar);
      ps_multiply(X, X, X2, 1.0, 0.0, p.threshold);
      fused = step && ps_saf_update(X, X2, -1.0 * alpha * alpha, 2 * alpha, WH, &dot, &trace_x);
      if (!fused) ps_axpby(X2, X, -1.0 * alpha * alpha, 2 * alpha, 0.0);   // ScaleMatrix(X, 2 alpha); IncrementMatrix(X2, X, -alpha^2)
      Beta = 2.0 * alpha * Beta - alpha * alpha * Beta * Beta;
      BetaBar = 2.0 * alpha * BetaBar - alpha * alpha * BetaBar * BetaBar;
    }
    if (!fused) {
      dot = real_dot(X, WH);
      trace_x = std::nan("");
    }
    if (f.converged(2.0 * dot, trace_value > trace ? -1.0 : 1.0, X)) break;
  }
  slab.close();
  ps_slab_leave(X);
  f.finish(II, X, ISQ, K, energy_out);                             // :1095-1101
}

// EnergyDensityMatrix (:1165-1187): ED = D H D
void energy_density_matrix(const PSMatrix& H, const PSMatrix& D, PSMatrix& ED, double threshold) {
  CommScope cs(H.grid);
  ps_similarity(H, D, D, ED, threshold);
}

// McWeenyStep (:1190-1231): DOut = 3 DSD - 2 DSDSD
void mcweeny_step(const PSMatrix& D, PSMatrix& DOut, const PSMatrix* S, double threshold) {
  CommScope cs(D.grid);
  PSMatrix DS, DSD;
  if (S) ps_multiply(D, *S, DS, 1.0, 0.0, threshold);
  else ps_copy(D, DS);
  ps_multiply(DS, D, DSD, 1.0, 0.0, threshold);
  PSMatrix Out;
  ps_multiply(DS, DSD, Out, -2.0, 0.0, threshold);
  ps_increment(DSD, Out, 3.0, 0.0);
  DOut.grid = Out.grid; DOut.dim = Out.dim; DOut.cplx = Out.cplx; DOut.c0 = Out.c0; DOut.c1 = Out.c1;
  DOut.loc = std::move(Out.loc);
}

// ------------------------------------------------------------------ Sign / Polar
namespace {
// CoreComputation (SignSolversModule.F90:150-258)
void sign_core(const PSMatrix& InMat, PSMatrix& OutMat, const SolverParameters& p, bool needs_transpose) {
  const double alpha = 1.69770248526;
  Monitor mon;
  monitor_construct(mon, p.monitor_convergence, p.converge_diff);
  PSMatrix Identity, Temp1, Temp2, OutMatT, Out;
  ps_construct_like(Identity, InMat);
  ps_fill_identity(Identity);
  balance_permute(Identity, p);
  balance_copy(InMat, Out, p);
  double e_min, e_max;
  ps_gershgorin(InMat, &e_min, &e_max);
  double xk = std::fabs(e_min / e_max);
  ps_scale(Out, 1.0 / std::fabs(e_max));
  log_iterations_header(p);
  int II;
  // (complex operands under FMA arithmetic: the loop's products, identity increment and norm take them in slab form as well)
  const bool complex_session = complex_slab_loop(Out);
  // (PolarDecomposition: the loop transposes its iterate, which a session keeps in slab form only under option slab_transpose --
  // one rank without process slices; 1: real operands, 2: complex ones as well.  Several ranks: compressed columns, as ever)
  const bool polar_ok = options().slab_transpose >= 1 && !world().active() && !(Out.grid && Out.grid->num_slices > 1) &&
                        (!Out.cplx || (options().slab_transpose >= 2 && complex_session));
  SlabSession slab((!needs_transpose || polar_ok) && (!Out.cplx || complex_session), false, complex_session);
  if (needs_transpose && slab.opened) {
    slab_transpose_counts()[3] += 1;
    slab_keep_sparse_runs(true);   // (unfused arithmetic: no product of this loop leaves slab form for the general kernels)
  }
  for (II = 1; II <= p.max_iterations; ++II) {
    const double alpha_k = std::fmin(std::sqrt(3.0 / (1.0 + xk + xk * xk)), alpha);
    xk = 0.5 * alpha_k * xk * (3.0 - (alpha_k * alpha_k) * (xk * xk));
    if (needs_transpose) {
      ps_transpose(Out, OutMatT);
      if (OutMatT.cplx) ps_conjugate(OutMatT);
      ps_multiply(OutMatT, Out, Temp1, -1.0 * (alpha_k * alpha_k), 0.0, p.threshold);
    } else {
      ps_multiply(Out, Out, Temp1, -1.0 * (alpha_k * alpha_k), 0.0, p.threshold);
    }
    ps_increment_identity(Identity, Temp1, 3.0);                   // IncrementMatrix(Identity, Temp1, 3)
    ps_multiply(Out, Temp1, Temp2, 0.5 * alpha_k, 0.0, p.threshold);
    double norm_value = 0.0;   // (the difference Out - Temp2 is only there for its norm)
    if (!ps_norm_axpby(Temp2, Out, -1.0, 1.0, &norm_value)) {
      ps_increment(Temp2, Out, -1.0, 0.0);
      norm_value = ps_norm(Out);
    }
    std::swap(Out.loc, Temp2.loc);   // CopyMatrix(Temp2, Out): Temp2 is rebuilt by the next multiply
    monitor_append(mon, norm_value);
    trace_rec(norm_value, 0.0, alpha_k, Out);
    if (monitor_converged(mon, p.be_verbose)) break;
  }
  slab.close();
  ps_slab_leave(Out);
  if (p.be_verbose) {
    log_exit();
    log_element("Total Iterations", II - 1);
    print_matrix_information(Out);
  }
  balance_undo(Out, p);
  OutMat = std::move(Out);
}
}  // namespace

void solver_sign(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p) {
  CommScope cs(A.grid);
  if (band_scope_try({&A}, {&Out}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) { solver_sign(*in[0], *out[0], p); }))
    return;
  trace_reset();
  solver_header("Sign Function Solver", "nicholas2008functions", p);
  sign_core(A, Out, p, false);
  if (p.be_verbose) log_exit();
}

void solver_polar(const PSMatrix& A, PSMatrix& U, PSMatrix* Hm, const SolverParameters& p) {
  CommScope cs(A.grid);
  trace_reset();
  solver_header("Polar Decomposition Solver", "nicholas2008functions", p);
  sign_core(A, U, p, true);
  if (Hm) {  // SignSolversModule.F90:129-137
    PSMatrix UT;
    ps_transpose(U, UT);
    if (UT.cplx) ps_conjugate(UT);
    ps_multiply(UT, A, *Hm, 1.0, 0.0, p.threshold);
  }
  if (p.be_verbose) log_exit();
}

// ------------------------------------------------------------------ Invert / PseudoInverse
namespace {
void invert_core(const PSMatrix& InputMat, PSMatrix& OutputMat, const SolverParameters& p, bool log_top) {
  Monitor mon;
  monitor_construct(mon, p.monitor_convergence, p.converge_diff);
  solver_header("Inverse Solver", "palser1998canonical", p);
  PSMatrix Temp1, Temp2, Identity, Balanced, Out;
  ps_construct_like(Identity, InputMat);
  ps_fill_identity(Identity);
  balance_permute(Identity, p);
  balance_copy(InputMat, Balanced, p);
  const double sigma = ps_sigma(Balanced);
  ps_copy(Balanced, Out);
  ps_scale(Out, sigma);
  log_iterations_header(p);
  double norm_value = p.converge_diff + 1.0;
  int II;
  // (complex operands under FMA arithmetic: products, merges, scalings, copies and norms take them in slab form as well)
  const bool complex_session = complex_slab_loop(Out);
  SlabSession slab(!Out.cplx || complex_session, false, complex_session);
  for (II = 1; II <= p.max_iterations; ++II) {
    if (log_top && p.be_verbose && II > 1) log_list_element("Convergence", norm_value);
    ps_multiply(Out, Balanced, Temp1, 1.0, 0.0, p.threshold);
    if (!ps_norm_axpby(Temp1, Identity, -1.0, 1.0, &norm_value)) {   // (I - Temp1 is only there for its norm)
      ps_copy_axpby(Identity, Temp1, Temp2, -1.0, 1.0, 0.0);       // CopyMatrix(Identity, Temp2); IncrementMatrix(Temp1, Temp2, -1)
      norm_value = ps_norm(Temp2);
    }
    PSMatrix T2;
    ps_multiply(Temp1, Out, T2, -1.0, 0.0, p.threshold);
    ps_axpby(T2, Out, 1.0, 2.0, p.threshold);                       // ScaleMatrix(Out, 2); IncrementMatrix(T2, Out)
    monitor_append(mon, norm_value);
    trace_rec(norm_value, 0.0, sigma, Out);
    if (monitor_converged(mon, p.be_verbose)) break;
  }
  slab.close();
  ps_slab_leave(Out);
  if (p.be_verbose) {
    log_exit();
    log_element("Total Iterations", II - 1);
    print_matrix_information(Out);
  }
  balance_undo(Out, p);
  if (p.be_verbose) log_exit();
  OutputMat = std::move(Out);
}
}  // namespace

void solver_invert(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p) {
  CommScope cs(A.grid);
  if (band_scope_try({&A}, {&Out}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) { solver_invert(*in[0], *out[0], p); }))
    return;
  trace_reset();
  invert_core(A, Out, p, true);
}
void solver_pseudoinverse(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p) {
  CommScope cs(A.grid);
  if (band_scope_try({&A}, {&Out}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) { solver_pseudoinverse(*in[0], *out[0], p); }))
    return;
  trace_reset();
  invert_core(A, Out, p, false);
}

// ------------------------------------------------------------------ (inverse) square root
namespace {
// NewtonSchultzISROrder2 (SquareRootSolversModule.F90:198-338)
void isr_order2(const PSMatrix& InMat, PSMatrix& OutMat, const SolverParameters& p, bool compute_inverse) {
  Monitor mon;
  monitor_construct(mon, p.monitor_convergence, p.converge_diff);
  solver_header("Newton Schultz Inverse Square Root", "jansik2007linear", p);
  PSMatrix X, T, Temp, Identity, SR, ISR;
  ps_construct_like(Identity, InMat);
  ps_fill_identity(Identity);
  double e_min, e_max;
  ps_gershgorin(InMat, &e_min, &e_max);
  double max_between = std::fmax(std::fabs(e_min), std::fabs(e_max));
  double lambda = 1.0 / max_between;
  ps_construct_like(ISR, InMat);
  ps_fill_identity(ISR);
  ps_copy(InMat, SR);
  balance_permute(SR, p);
  balance_permute(Identity, p);
  balance_permute(ISR, p);
  log_iterations_header(p);
  int II;
  SlabSession slab(!SR.cplx);
  for (II = 1; II <= p.max_iterations; ++II) {
    ps_multiply(SR, ISR, X, 1.0, 0.0, p.threshold);
    ps_gershgorin(X, &e_min, &e_max);
    max_between = std::fmax(std::fabs(e_min), std::fabs(e_max));
    lambda = 1.0 / max_between;
    ps_scale(X, lambda);
    double norm_value = 0.0;   // (I - X is only there for its norm: Temp is handed over as storage below)
    if (!ps_norm_axpby(X, Identity, -1.0, 1.0, &norm_value)) {
      ps_copy_axpby(Identity, X, Temp, -1.0, 1.0, 0.0);             // CopyMatrix(Identity, Temp); IncrementMatrix(X, Temp, -1)
      norm_value = ps_norm(Temp);
    }
    ps_copy_axpby(Identity, X, T, -1.0, 3.0, 0.0);                  // CopyMatrix(Identity, T); ScaleMatrix(T, 3); IncrementMatrix(X, T, -1)
    ps_scale(T, 0.5);
    std::swap(ISR, Temp);                                           // CopyMatrix(ISR, Temp): ISR is rebuilt by the multiply
    ps_multiply(Temp, T, ISR, 1.0, 0.0, p.threshold);
    ps_scale(ISR, std::sqrt(lambda));
    std::swap(SR, Temp);
    ps_multiply(T, Temp, SR, 1.0, 0.0, p.threshold);
    ps_scale(SR, std::sqrt(lambda));
    monitor_append(mon, norm_value);
    trace_rec(norm_value, 0.0, lambda, ISR);
    if (monitor_converged(mon, p.be_verbose)) break;
  }
  slab.close();
  ps_slab_leave(ISR);
  ps_slab_leave(SR);
  if (p.be_verbose) {
    log_exit();
    log_element("Total Iterations", II);
    print_matrix_information(ISR);
  }
  PSMatrix Out;
  ps_copy(compute_inverse ? ISR : SR, Out);
  balance_undo(Out, p);
  if (p.be_verbose) log_exit();
  OutMat = std::move(Out);
}

// NewtonSchultzISRTaylor (SquareRootSolversModule.F90:342-531)
void isr_taylor(const PSMatrix& InMat, PSMatrix& OutMat, const SolverParameters& p, int order, bool compute_inverse) {
  Monitor mon;
  monitor_construct(mon, p.monitor_convergence, p.converge_diff);
  solver_header("Newton Schultz Inverse Square Root", "jansik2007linear", p);
  PSMatrix X, Temp, Temp2, Identity, SR, ISR;
  ps_construct_like(Identity, InMat);
  ps_fill_identity(Identity);
  double e_min, e_max;
  ps_gershgorin(InMat, &e_min, &e_max);                            // :389-391
  const double max_between = std::fmax(std::fabs(e_min), std::fabs(e_max));
  const double lambda = 1.0 / max_between;
  ps_construct_like(ISR, InMat);                                   // :394-396
  ps_fill_identity(ISR);
  ps_copy(InMat, SR);
  ps_scale(SR, lambda);
  balance_permute(SR, p);                                          // :399-406
  balance_permute(Identity, p);
  balance_permute(ISR, p);
  log_iterations_header(p);
  int II;
  // (complex operands under FMA arithmetic: the loop's whole vocabulary takes them in slab form -- SquareRootSolversModule.F90:415-497)
  const bool complex_session = complex_slab_loop(SR);
  SlabSession slab(!SR.cplx || complex_session, false, complex_session);
  for (II = 1; II <= p.max_iterations; ++II) {                     // :415-497
    ps_multiply(ISR, SR, X, 1.0, 0.0, p.threshold);
    ps_increment_identity(Identity, X, -1.0);
    const double norm_value = ps_norm(X);
    if (order == 3) {                                              // :425-433
      ps_multiply(X, X, Temp, 1.0, 0.0, p.threshold);
      if (!ps_isr_chain3(X, Temp)) {                                // (option isr_chain: the two merges in one pass over X and X X)
        ps_axpby(Identity, X, 1.0, -0.5, 0.0);                      // ScaleMatrix(X, -1/2); IncrementMatrix(I, X)
        ps_increment(Temp, X, 0.375, 0.0);
      }
    } else {                                                       // :434-479 (Knuth's 2-multiply quartic)
      const double aa = -40.0 / 35.0, bb = 48.0 / 35.0, cc = -64.0 / 35.0, dd = 128.0 / 35.0;
      const double a = (aa - 1.0) / 2.0;
      const double b = bb * (a + 1.0) - cc - a * ((a + 1.0) * (a + 1.0));
      const double c = bb - b - a * (a + 1.0);
      const double d = dd - b * c;
      ps_multiply(X, X, Temp, 1.0, 0.0, p.threshold);
      if (!ps_isr_chain5(X, Temp, a, b, c, Temp2, Temp)) {          // (option isr_chain: the four calls in one pass over X and X X)
        ps_increment(X, Temp, a, 0.0);
        ps_copy_axpby(Identity, X, Temp2, 1.0, b, 0.0);             // CopyMatrix(Identity, Temp2); ScaleMatrix(Temp2, b); IncrementMatrix(X, Temp2)
        ps_increment(Temp, Temp2, 1.0, 0.0);
        ps_increment_identity(Identity, Temp, c);
      }
      ps_multiply(Temp2, Temp, X, 1.0, 0.0, p.threshold);
      ps_increment_identity(Identity, X, d);
      ps_scale(X, 35.0 / 128.0);
    }
    std::swap(ISR, Temp);                                          // :483-485 (the copy is a hand-over: ISR is rebuilt)
    ps_multiply(X, Temp, ISR, 1.0, 0.0, p.threshold);
    std::swap(SR, Temp);                                           // :488-490
    ps_multiply(Temp, X, SR, 1.0, 0.0, p.threshold);
    monitor_append(mon, norm_value);
    trace_rec(norm_value, 0.0, lambda, ISR);
    if (monitor_converged(mon, p.be_verbose)) break;
  }
  slab.close();
  ps_slab_leave(ISR);
  ps_slab_leave(SR);
  if (p.be_verbose) {
    log_exit();
    log_element("Total Iterations", II);
    print_matrix_information(ISR);
  }
  PSMatrix Out;
  if (compute_inverse) {                                           // :505-511
    ps_scale(ISR, std::sqrt(lambda));
    ps_copy(ISR, Out);
  } else {
    ps_scale(SR, 1.0 / std::sqrt(lambda));
    ps_copy(SR, Out);
  }
  balance_undo(Out, p);
  if (p.be_verbose) log_exit();
  OutMat = std::move(Out);
}
}  // namespace

void solver_square_root(const PSMatrix& A, PSMatrix& Out, const SolverParameters& p, bool inverse, int order) {
  CommScope cs(A.grid);
  if (band_scope_try({&A}, {&Out}, [&](const std::vector<const PSMatrix*>& in, const std::vector<PSMatrix*>& out) { solver_square_root(*in[0], *out[0], p, inverse, order); }))
    return;
  trace_reset();
  // SquareRootSelector (SquareRootSolversModule.F90:164-194): default order 5
  if (order == 2) isr_order2(A, Out, p, inverse);
  else isr_taylor(A, Out, p, order == 3 ? 3 : 5, inverse);
}

}  // namespace ntp
