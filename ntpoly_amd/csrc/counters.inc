// The counter arrays the C ABI exposes, one entry each: NTP_COUNTER(name, N, accessor) is the entry point
// void ntpoly_amd_<name>_counts(long long out[N]), which copies accessor()[0 .. N) into out.  wrp.cpp generates the entry points
// from this table, tools/gen_headers.py their prototypes in include/ntpoly_amd.h; ntpoly_amd/host.py names the slots in its own
// table (_COUNTERS).  The arrays and their accessors stay with the code that counts.  Every count is cumulative since the start
// of the process unless its entry says otherwise.
// To add a counter: one entry here, one in host.py's table, then regenerate the headers (DESIGN.md, "Adding an option, adding a counter").

// groups finished by the grouped LDS-hash kernel (spgemm_grouped.hip), by path: [0] real operands on the matrix cores (option
// ghash_mfma), [1] real on the vector units, [2] complex on the matrix cores (option ghash_mfma_complex: table class 0 in FMA
// arithmetic with complex_tile), [3] complex on the vector units
NTP_COUNTER(ghash_class, 4, ghash_class_counts)
// products of slab sessions computed by the thin-operand gather kernels (spgemm_thin.hip): [0] real, thin left operand; [1] real,
// thin right; [2] complex left; [3] complex right; of those, panel products (slab sessions on several ranks): [4] real, [5] complex
NTP_COUNTER(thin_slab, 6, thin_slab_counts)
// The polynomial chain of the Taylor square-root step in one pass (option isr_chain; engine.hpp ps_isr_chain5 / ps_isr_chain3):
// [0] order-5 chains fused, [1] order-3 chains fused, [2] chains refused (the vocabulary calls ran instead).  A step that never
// reaches the kernel's decision -- the option off, no session for the operands' kind, X and X X both in compressed columns
// (unfused arithmetic near convergence), a labelled slab form -- is neither fused nor counted as refused
NTP_COUNTER(isr_chain, 3, isr_chain_counts)
// The transpose of a slab form (option slab_transpose; engine.hpp ps_transpose / ps_conjugate): [0] transposes done in slab form,
// [1] conjugations done in slab form, [2] transposes refused past the gates (extents far apart: that one ran on compressed
// columns), [3] PolarDecomposition solves that ran in a slab session.  A gated operand -- no session, several ranks, compressed
// columns, a view, a labelled form, block form -- counts nowhere
NTP_COUNTER(slab_transpose, 4, slab_transpose_counts)
// PowerBounds on one vector (option power_vector; engine.hpp ps_power_vector_open / ps_power_vector_step): [0] PowerBounds solves
// that ran on one vector, [1] power steps computed by k_pv_step, [2] solves that passed the gates but were refused (the gather form
// could not be built: the N-column loop ran).  A solve kept out by a gate -- the option off, process slices > 1 -- counts nowhere;
// the diagnostic entry point ntpoly_amd_power_vector_step counts nothing
NTP_COUNTER(power_vector, 3, power_vector_counts)
// CGSolver with its traces from column dot passes (option cg_dots; engine.hpp ps_cg_dots): [0] solves that ran with the passes, [1]
// dot passes done by k_cg_dots, [2] passes refused past the gates (the same chains ran on the rank's compressed columns), [3]
// products and transposes not formed.  A solve kept out by a gate -- the option off, no session for the operands' kind, block
// form, process slices > 1, complex operands with the option below 2 or on several ranks -- counts nowhere; the diagnostic entry
// point ntpoly_amd_cg_dots counts nothing
NTP_COUNTER(cg_dots, 4, cg_dots_counts)
// WOM_GC / WOM_C in a slab session (option wom_session; engine.hpp ps_wom_heun / ps_wom_c_dots): [0] solves that ran in a slab
// session, [1] Heun tails fused (k_wom_heun), [2] pairs of dots of the canonical step fused (k_wom_c_dots), [3] passes refused past
// the gates (the vocabulary calls ran instead).  A pass kept out by a gate -- the option below 2, no open real session, a complex
// operand, block form, a labelled slab form, dimensions that differ, one matrix given twice -- counts nowhere
NTP_COUNTER(wom_session, 4, wom_session_counts)
// PurificationExtrapolate in a slab session (option purify_session; engine.hpp ps_purify_tail): [0] solves that ran in a slab
// session, [1] tails fused in the fold branch (k_purify_tail writes N' = 2 D - D S D), [2] tails fused in the plain branch (nothing
// written), [3] passes refused past the gates (the vocabulary calls ran instead).  A pass kept out by a gate -- the option below 2,
// no open real session, a complex operand, block form, a labelled slab form, dimensions that differ, one matrix given twice --
// counts nowhere
NTP_COUNTER(purify_session, 4, purify_session_counts)
// ComputeExponentialPade in a slab session (option pade_session; engine.hpp ps_pade_chain): [0] calls that ran in a slab session,
// [1] sum passes fused (k_pade_chain<3> writes P1 and TempMat), [2] pair passes fused (k_pade_chain<1> writes LeftMat and RightMat),
// [3] passes refused past the gates (the vocabulary calls ran instead).  A pass kept out by a gate -- the option below 2, no open
// real session, a complex operand, block form, a labelled slab form, dimensions that differ, one matrix given twice, a number of
// addends other than 1 or 3 -- counts nowhere
NTP_COUNTER(pade_session, 4, pade_session_counts)
// The real Chebyshev / Hermite step in one pass and ComputeExponential's squarings in a slab session (option poly_step; engine.hpp
// ps_poly_step): [0] ComputeExponential calls whose real squarings ran in a slab session, [1] steps fused (k_poly_step writes Tk
// and the new sum), [2] passes refused past the gates (the two merges ran instead).  A step kept out by a gate -- the option
// below 2, no open real session, a complex operand, block form, a labelled slab form, dimensions that differ, one matrix in two
// roles, a zero coefficient, a grid with process slices -- counts nowhere
NTP_COUNTER(poly_step, 3, poly_step_counts)
// The scaled sum chain of the real solver loops in one pass (option sum_chain; engine.hpp ps_sum_chain): [0] passes fused
// (k_sum_chain<M> writes the sum), [1] passes refused past the gates (the vocabulary calls ran instead).  A pass kept out by a
// gate -- the option at 0, no open real session or one that has given up, a complex operand, block form, a labelled slab form,
// dimensions that differ, one matrix in two input roles, the output among the addends, a number of addends outside 1 .. 5, a
// grid with process slices, a scalar that is zero or not finite -- counts nowhere
NTP_COUNTER(sum_chain, 2, sum_chain_counts)
// The complex side of the sum chain (option complex_sum_chain; engine.hpp ps_sum_chain on complex operands): [0] inverse-root
// loops that opened a complex slab session (level 1; a loop that runs inside an outer session which already takes complex
// operands stays in slab form too, but opens nothing and is not counted), [1] passes fused (k_sum_chain<double2, M> writes the sum; level 2), [2] passes
// refused past the gates (the vocabulary calls ran instead).  A pass kept out by a gate -- the option below 2, no open session that
// takes complex operands or one that has given up, block form, a labelled slab form, dimensions that differ, one matrix in two
// input roles, the output among the addends, a number of addends outside 1 .. 5, a grid with process slices, real and complex
// operands mixed, a scalar that is zero or not finite -- counts nowhere.  Real operands count in sum_chain only, complex ones here only
NTP_COUNTER(complex_sum_chain, 3, complex_sum_chain_counts)
// HPCP purification with its traces and its update in one pass each (option hpcp_step; engine.hpp ps_hpcp_traces / ps_hpcp_update):
// [0] trace passes fused, [1] updates fused, [2] updates refused (the vocabulary calls ran instead).  A step that never reaches
// the kernel's decision -- the option off, no open real session, a complex operand, block form, a labelled slab form, alignments
// that differ, a WH the dot cannot read as runs -- is neither fused nor counted as refused
NTP_COUNTER(hpcp_step, 3, hpcp_step_counts)
// Complex HPCP in a complex slab session (option complex_hpcp; engine.hpp ps_hpcp_traces / ps_hpcp_update on complex operands):
// [0] trace passes fused, [1] updates fused, [2] passes refused (the vocabulary calls ran instead).  A pass that never reaches
// the kernel's decision -- the option off, no open complex session, several ranks, block form, a labelled slab form, alignments
// that differ, a WH the dot cannot read as runs -- is neither fused nor counted as refused.  Real operands count in hpcp_step
// only, complex ones here only.  With the option on, ntpoly_amd_hpcp_update_step takes four complex matrices in a session with
// complex_ok: the chain on each part of an entry, *energy = the real part of DotMatrix
NTP_COUNTER(complex_hpcp, 3, complex_hpcp_counts)
// ScaleAndFold with the update, the energy and the next step's trace in one pass (option scale_fold_step; engine.hpp ps_saf_update /
// ps_saf_dot_trace): [0] fold updates fused, [1] dot-and-trace passes fused (the scale branch), [2] passes refused (the vocabulary
// calls ran instead).  A step that never reaches the kernel's decision -- the option off, no open real session, a complex
// operand, block form, a labelled slab form, alignments that differ, a WH the dot cannot read as runs -- is neither fused nor
// counted as refused
NTP_COUNTER(scale_fold_step, 3, scale_fold_step_counts)
// Complex ScaleAndFold in a complex slab session (option complex_scale_fold; engine.hpp ps_saf_update / ps_saf_dot_trace on complex
// operands): [0] fold updates fused, [1] dot-and-trace passes fused (the scale branch), [2] passes refused (the vocabulary calls
// ran instead).  A pass that never reaches the kernel's decision -- the option off, no open complex session, several ranks, block
// form, a labelled slab form, alignments that differ, a WH the dot cannot read -- is neither fused nor counted as refused.  Real
// operands count in scale_fold_step only, complex ones here only.  With the option on, ntpoly_amd_scale_fold_update_step and
// ntpoly_amd_scale_fold_dot_trace take complex matrices in a session with complex_ok: *dot = the real part of DotMatrix, *trace =
// MatrixTrace
NTP_COUNTER(complex_scale_fold, 3, complex_scale_fold_counts)
// Complex TRS4 in a complex slab session (option complex_trs4; engine.hpp ps_trs4_traces / ps_trs4_operand / ps_trs4_energy on
// complex operands): [0] trace passes fused, [1] operands Fx + sigma Gx fused, [2] energies fused, [3] passes refused (the
// vocabulary calls ran instead).  A pass that never reaches the kernel's decision -- the option off, no open complex session,
// several ranks, block form, a labelled slab form -- is neither fused nor counted as refused
NTP_COUNTER(complex_trs4, 4, complex_trs4_counts)
// PM purification on a slab-form iterate (option pm_session; engine.hpp ps_pm_sigma / ps_pm_update): [0] sigma passes fused, [1]
// updates fused, [2] stored zeros carried beside the runs (summed over the updates), [3] solves that left the fused path.  The
// array's fifth slot, the longest zero list an update left on this rank, has its own entry point (ntpoly_amd_pm_session_longest_list)
NTP_COUNTER(pm_session, 4, pm_session_counts)
// Complex PM in a complex slab session (option complex_pm; engine.hpp ps_pm_sigma / ps_pm_update on complex operands): [0] sigma
// passes fused, [1] updates fused, [2] stored (0, 0) entries carried beside the runs (summed over the updates), [3] solves that
// left the fused path.  A solve that a gate keeps out -- the option off, several ranks, iterates in block form -- counts nowhere.
// Real operands count in pm_session only, complex ones here only
NTP_COUNTER(complex_pm, 4, complex_pm_counts)
// purification steps computed inside the SpGEMM kernel's epilogue: [0] steps with SlabFusion mode 1 (X*X), [1] mode 2 (2X - X*X),
// [2] fused steps that had to be repeated on the unfused path
NTP_COUNTER(fusion, 3, fusion_counts)
// complex TRS2 steps done in complex slab or block form (product, merge and energy pass; not a fused tile epilogue): [0] X*X,
// [1] 2X - X*X, [2] steps that had to be repeated the old way
NTP_COUNTER(complex_fusion, 3, complex_fusion_counts)
// [0] multiplies computed in the two-block geometry of the MFMA kernel (spgemm_tile2.hip), [1] launches of it whose geometry did
// not fit after all and were repeated on k_spgemm_tile
NTP_COUNTER(tile2, 2, tile2_counts)
// since the last ntpoly_amd_reset_spgemm_accum: [0] tiles the MFMA tile kernel tested against the operand's segment maxima
// (option tile_skip), [1] tiles it skipped
NTP_COUNTER(tile_skip, 2, tile_skip_counts)
// [0] solves that ran in a recovered band order across ranks (band_scope.cpp), [1] operands searched for one.  (The array's third
// slot, solves in a BLOCK order, is read by ntpoly_amd_block_scope_counts)
NTP_COUNTER(band_scope, 2, band_scope_counts)
// operations on compressed columns without the merge pass (column_fused.hip): [0] IncrementMatrix(Identity, .) done in place,
// [1] norms of differences taken from the operands without forming them
NTP_COUNTER(column_fused, 2, column_fused_counts)
// [0] vocabulary operations (copy, scale, merge, dot, trace, norm) done on matrices in block form (spgemm_block.hpp block
// algebra), [1] fallbacks to compressed columns
NTP_COUNTER(block_algebra, 2, block_algebra_counts)
// operations the solver loops did on matrices in slab form: [0] products, [1] merges / copies, [2] other operations (scalings /
// dots / norms); [3] operations that had to go back to compressed columns
NTP_COUNTER(slab_algebra, 4, slab_algebra_counts)
// read-only slab views of operands with stored zeros (option stored_zero_views), real and complex: [0] views built from compressed
// columns, [1] products with a view operand done in slab form, [2] merges / copies / scalings with a view operand done in slab
// form, [3] merges on a view declined because the result would hold a stored zero (done on compressed columns instead)
NTP_COUNTER(slab_view, 4, slab_view_counts)
// products of slab sessions on more than one rank: [0] done in slab form on every rank, [1] declined (compressed columns), [2] host
// synchronisations inside the former (measured)
NTP_COUNTER(panel_product, 3, panel_product_counts)
