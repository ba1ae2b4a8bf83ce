// Matrix polynomials: host-side callers of the distributed algebra.
//   PolynomialSolversModule.F90  : Horner (Compute_stand :74-161), Paterson-Stockmeyer (FactorizedCompute_stand :165-282)
//   ChebyshevSolversModule.F90   : three-term recurrence (Compute_cheby :69-160), divide and conquer
//                                  (FactorizedCompute_cheby :163-247 + ComputeRecursive :250-365)
//   HermiteSolversModule.F90     : physicists' Hermite recurrence (Compute_horner :52-184)
// Same control flow, same order of operations, same use (or, for Paterson-Stockmeyer, non-use) of the threshold.
#include <cmath>
#include <vector>

#include "engine.hpp"

namespace ntp {

namespace {
struct Balanced {  // identity + input, permuted when load balancing is on (the common preamble of these solvers)
  PSMatrix Identity, Input;
};
void balanced_setup(const PSMatrix& In, const SolverParameters& p, Balanced& b) {
  ps_construct_like(b.Identity, In);
  ps_fill_identity(b.Identity);
  ps_copy(In, b.Input);
  balance_permute(b.Identity, p);
  balance_permute(b.Input, p);
}
// the evaluation's session: real operands as ever; complex ones in slab form too where the loop may take them (option
// complex_poly_sessions, on top of what the sign loop's complex session needs)
bool complex_poly_session(const PSMatrix& In) { return complex_slab_loop(In) && options().complex_poly_sessions != 0; }
void poly_header(const char* solver, const char* method, const char* citation, int degree, const SolverParameters& p,
                 bool degree_first) {
  if (!p.be_verbose) return;
  log_header(solver);
  log_enter();
  log_element("Method", method);
  if (citation) log_citations({citation});
  if (degree_first) log_element("Degree", degree - 1);
  print_parameters(p);
  if (!degree_first) log_element("Degree", degree - 1);
}
}  // namespace

// ------------------------------------------------------------------ Horner
void polynomial_horner(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p) {
  CommScope cs(In.grid);
  const int degree = (int)c.size();
  if (degree < 1) NTP_FATAL("polynomial without coefficients");
  poly_header("Polynomial Solver", "Horner", nullptr, degree, p, false);
  Balanced b;
  balanced_setup(In, p, b);
  const bool complex_session = complex_poly_session(In);
  SlabSession slab(!In.cplx || complex_session, false, complex_session);   // (engine.hpp: products, merges and scalings of the evaluation on matrices kept in slab form)
  PSMatrix R, Temporary;
  ps_copy(b.Identity, R);
  if (degree == 1) {
    ps_scale(R, c[(size_t)degree - 1]);
  } else {
    ps_scale(R, c[(size_t)degree - 2]);
    ps_increment(b.Input, R, c[(size_t)degree - 1], 0.0);
    for (int II = degree - 2; II >= 1; --II) {
      ps_multiply(b.Input, R, Temporary, 1.0, 0.0, p.threshold);
      std::swap(R.loc, Temporary.loc);
      ps_increment(b.Identity, R, c[(size_t)II - 1], 0.0);
    }
  }
  slab.close();
  ps_slab_leave(R);
  balance_undo(R, p);
  Out = std::move(R);
  if (p.be_verbose) log_exit();
}

// ------------------------------------------------------------------ Paterson-Stockmeyer
void polynomial_paterson_stockmeyer(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c,
                                    const SolverParameters& p) {
  CommScope cs(In.grid);
  const int degree = (int)c.size();
  if (degree < 2) NTP_FATAL("Paterson-Stockmeyer needs a polynomial of degree >= 1");
  const int m_value = degree - 1;
  const int s_value = (int)std::sqrt((float)m_value);
  const int r_value = m_value / s_value;
  poly_header("Polynomial Solver", "Paterson Stockmeyer", "paterson1973number", degree, p, false);
  PSMatrix Identity;
  ps_construct_like(Identity, In);
  ps_fill_identity(Identity);
  const bool complex_session = complex_poly_session(In);
  SlabSession slab(!In.cplx || complex_session, false, complex_session);
  std::vector<PSMatrix> x_powers((size_t)s_value + 1);
  ps_construct_like(x_powers[0], In);
  ps_fill_identity(x_powers[0]);
  for (int II = 1; II <= s_value; ++II)  // no threshold here (the reference passes none, :229-232)
    ps_multiply(In, x_powers[(size_t)II - 1], x_powers[(size_t)II], 1.0, 0.0, 0.0);
  PSMatrix Xs, Bk, R, Temp;
  ps_copy(x_powers[(size_t)s_value], Xs);
  auto coef = [&](int one_based) { return c[(size_t)one_based - 1]; };
  // (option sum_chain, real operands: Bk = coef I + sum of `count` scaled powers in one pass, engine.hpp ps_sum_chain; a group
  // without an addend, with more than five or with a zero coefficient is kept out by its gates and takes the calls)
  auto bk_chain = [&](int k, int count) {
    std::vector<const PSMatrix*> powers;
    std::vector<double> weights;
    for (int II = 1; II <= count; ++II) {
      powers.push_back(&x_powers[(size_t)II]);
      weights.push_back(coef(s_value * k + II + 1));
    }
    return ps_sum_chain(Identity, coef(s_value * k + 1), powers.data(), weights.data(), count, 1.0, Bk);
  };

  if (!bk_chain(r_value, m_value - s_value * r_value)) {
    ps_copy(Identity, Bk);
    ps_scale(Bk, coef(s_value * r_value + 1));
    for (int II = 1; II <= m_value - s_value * r_value; ++II) {
      const int c_index = s_value * r_value + II;
      ps_increment(x_powers[(size_t)II], Bk, coef(c_index + 1), 0.0);
    }
  }
  ps_multiply(Bk, Xs, R, 1.0, 0.0, 0.0);

  int k_value = r_value - 1;
  if (!bk_chain(k_value, s_value - 1)) {
    ps_copy(Identity, Bk);
    ps_scale(Bk, coef(s_value * k_value + 1));
    for (int II = 1; II <= s_value - 1; ++II) {
      const int c_index = s_value * k_value + II;
      ps_increment(x_powers[(size_t)II], Bk, coef(c_index + 1), 0.0);
    }
  }
  ps_increment(Bk, R, 1.0, 0.0);

  for (k_value = r_value - 2; k_value >= 0; --k_value) {
    if (!bk_chain(k_value, s_value - 1)) {
      ps_copy(Identity, Bk);
      ps_scale(Bk, coef(s_value * k_value + 1));
      for (int II = 1; II <= s_value - 1; ++II) {
        const int c_index = s_value * k_value + II;
        ps_increment(x_powers[(size_t)II], Bk, coef(c_index + 1), 0.0);
      }
    }
    ps_multiply(Xs, R, Temp, 1.0, 0.0, 0.0);
    std::swap(R.loc, Temp.loc);
    ps_increment(Bk, R, 1.0, 0.0);
  }
  slab.close();
  ps_slab_leave(R);
  ps_slab_leave(const_cast<PSMatrix&>(In));   // (the session may have turned the caller's operand into slab form where it was)
  Out = std::move(R);
  if (p.be_verbose) log_exit();
}

// ------------------------------------------------------------------ Chebyshev, three-term recurrence
void chebyshev_compute(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p, bool keep_slab_form) {
  CommScope cs(In.grid);
  const int degree = (int)c.size();
  if (degree < 1) NTP_FATAL("polynomial without coefficients");
  poly_header("Chebyshev Solver", "Standard", nullptr, degree, p, true);
  Balanced b;
  balanced_setup(In, p, b);
  const bool complex_session = complex_poly_session(In);
  SlabSession slab(!In.cplx || complex_session, false, complex_session);
  PSMatrix Tk, Tkminus1, Tkminus2, R;
  ps_copy(b.Identity, Tkminus2);
  if (degree == 1) {
    ps_copy(Tkminus2, R);
    ps_scale(R, c[0]);
  } else {
    ps_copy(b.Input, Tkminus1);
    ps_copy(Tkminus2, R);
    ps_scale(R, c[0]);
    ps_increment(Tkminus1, R, c[1], 0.0);
    if (degree > 2) {
      ps_multiply(b.Input, Tkminus1, Tk, 2.0, 0.0, p.threshold);
      // (the two merges in one pass: real operands with option poly_step = 2, complex ones in a complex session)
      if (!ps_poly_step(Tk, Tkminus2, Tk, R, -1.0, c[2]) && !ps_recurrence_step(Tk, Tkminus2, Tk, R, -1.0, c[2])) {
        ps_increment(Tkminus2, Tk, -1.0, 0.0);
        ps_increment(Tk, R, c[2], 0.0);
      }
      for (int II = 4; II <= degree; ++II) {
        std::swap(Tkminus2.loc, Tkminus1.loc);  // Tkminus2 <- Tkminus1
        std::swap(Tkminus1.loc, Tk.loc);        // Tkminus1 <- Tk (Tk now holds scratch)
        ps_multiply(b.Input, Tkminus1, Tk, 2.0, 0.0, p.threshold);
        if (!ps_poly_step(Tk, Tkminus2, Tk, R, -1.0, c[(size_t)II - 1]) && !ps_recurrence_step(Tk, Tkminus2, Tk, R, -1.0, c[(size_t)II - 1])) {
          ps_increment(Tkminus2, Tk, -1.0, 0.0);
          ps_increment(Tk, R, c[(size_t)II - 1], 0.0);
        }
      }
    }
  }
  slab.close();
  // (keep_slab_form: compute_exponential's outer session is open and squares the result next; it sets this only where no load
  // balancer's permutation has to be undone on compressed columns)
  if (!keep_slab_form) ps_slab_leave(R);
  if (p.be_verbose) print_matrix_information(R);
  balance_undo(R, p);
  Out = std::move(R);
  if (p.be_verbose) log_exit();
}

// ------------------------------------------------------------------ Chebyshev, divide and conquer
namespace {
void cheby_recursive(const std::vector<PSMatrix>& T, const std::vector<double>& c, PSMatrix& Out, int depth,
                     const SolverParameters& p) {
  const int n = (int)c.size();
  if (n == 1) {
    ps_copy(T[0], Out);
    ps_scale(Out, c[0]);
  } else if (n == 2) {
    // (option sum_chain, real operands: c0 T0 + c1 T1 in one pass, engine.hpp ps_sum_chain)
    const PSMatrix* const t1[1] = {&T[1]};
    if (!ps_sum_chain(T[0], c[0], t1, &c[1], 1, 1.0, Out)) {
      ps_copy(T[0], Out);
      ps_scale(Out, c[0]);
      ps_increment(T[1], Out, c[1], 0.0);
    }
  } else {
    const int mid = n / 2;
    std::vector<double> left(c.begin(), c.begin() + mid), right(c.begin() + mid, c.end());
    for (int II = 2; II <= (int)left.size(); ++II) left[(size_t)II - 1] -= c[(size_t)(n - II + 2) - 1];
    PSMatrix LeftMat, RightMat, R;
    cheby_recursive(T, left, LeftMat, depth + 1, p);
    const int full_midpoint = (int)T.size() - depth + 1;  // 1-based index into T_Powers
    cheby_recursive(T, right, RightMat, depth + 1, p);
    ps_multiply(T[(size_t)full_midpoint - 1], RightMat, R, 2.0, 0.0, p.threshold);
    // (both merges behind the product in one pass)
    const PSMatrix* const tail[2] = {&LeftMat, &T[(size_t)full_midpoint - 1]};
    const double tail_c[2] = {1.0, -1.0 * right[0]};
    if (!ps_sum_chain(R, 1.0, tail, tail_c, 2, 1.0, R)) {
      ps_increment(LeftMat, R, 1.0, 0.0);
      ps_increment(T[(size_t)full_midpoint - 1], R, -1.0 * right[0], 0.0);
    }
    Out = std::move(R);
  }
}
}  // namespace

void chebyshev_factorized(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p) {
  CommScope cs(In.grid);
  const int degree = (int)c.size();
  if (degree < 1) NTP_FATAL("polynomial without coefficients");
  poly_header("Chebyshev Solver", "Recursive", nullptr, degree, p, true);
  Balanced b;
  balanced_setup(In, p, b);
  const bool complex_session = complex_poly_session(In);
  SlabSession slab(!In.cplx || complex_session, false, complex_session);
  int log2degree = 1;
  while ((1 << log2degree) <= degree) ++log2degree;
  std::vector<PSMatrix> T((size_t)log2degree);
  PSMatrix R;
  ps_copy(b.Identity, T[0]);
  if (degree == 1) {
    ps_copy(T[0], R);
  } else {
    ps_copy(b.Input, T[1]);
    for (int II = 3; II <= log2degree; ++II) {
      ps_multiply(T[(size_t)II - 2], T[(size_t)II - 2], T[(size_t)II - 1], 2.0, 0.0, p.threshold);
      ps_increment(b.Identity, T[(size_t)II - 1], -1.0, 0.0);
    }
    cheby_recursive(T, c, R, 1, p);
  }
  slab.close();
  ps_slab_leave(R);
  if (p.be_verbose) print_matrix_information(R);
  balance_undo(R, p);
  Out = std::move(R);
  if (p.be_verbose) log_exit();
}

// ------------------------------------------------------------------ Hermite
void hermite_compute(const PSMatrix& In, PSMatrix& Out, const std::vector<double>& c, const SolverParameters& p) {
  CommScope cs(In.grid);
  const int degree = (int)c.size();
  if (degree < 1) NTP_FATAL("polynomial without coefficients");
  poly_header("Hermite Solver", "Standard", nullptr, degree, p, true);
  Balanced b;
  balanced_setup(In, p, b);
  const bool complex_session = complex_poly_session(In);
  SlabSession slab(!In.cplx || complex_session, false, complex_session);
  PSMatrix Hk, Hkminus1, Hkplus1, Hkprime, R;
  ps_copy(b.Identity, Hkminus1);
  ps_copy(Hkminus1, R);
  ps_scale(R, c[0]);
  if (degree > 1) {
    ps_copy(b.Input, Hk);
    ps_scale(Hk, 2.0);
    ps_increment(Hk, R, c[1], 0.0);
    if (degree > 2) {
      ps_copy(Hkminus1, Hkprime);
      ps_scale(Hkprime, 2.0);
      for (int II = 3; II <= degree; ++II) {
        ps_multiply(b.Input, Hk, Hkplus1, 2.0, 0.0, p.threshold);
        // (HermiteSolversModule.F90:150-156: IncrementMatrix(Hkprime, Hkplus1, -1), two copies and a scaling of OTHER
        // matrices, IncrementMatrix(Hk = Hkplus1, OutputMat, c).  Hkprime already carries the coefficient 2 (k - 1), so the
        // recurrence's -2 (k - 1) H_{k-1} is a = -1 here; nothing between the two merges reads or writes Hkplus1 or the
        // output, so the second merge done right behind the first leaves the same values)
        const bool stepped = ps_poly_step(Hkplus1, Hkprime, Hkplus1, R, -1.0, c[(size_t)II - 1]) ||
                             ps_recurrence_step(Hkplus1, Hkprime, Hkplus1, R, -1.0, c[(size_t)II - 1]);
        if (!stepped) ps_increment(Hkprime, Hkplus1, -1.0, 0.0);
        ps_copy(Hk, Hkprime);
        ps_scale(Hkprime, (double)(2 * (II - 1)));
        std::swap(Hkminus1.loc, Hk.loc);   // Hkminus1 <- Hk
        std::swap(Hk.loc, Hkplus1.loc);    // Hk <- Hkplus1
        if (!stepped) ps_increment(Hk, R, c[(size_t)II - 1], 0.0);
      }
    }
  }
  slab.close();
  ps_slab_leave(R);
  if (p.be_verbose) print_matrix_information(R);
  balance_undo(R, p);
  Out = std::move(R);
  if (p.be_verbose) log_exit();
}

}  // namespace ntp
