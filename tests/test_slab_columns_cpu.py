"""CPU: the fused slab merge passes keep their public surface while their column sweep lives in csrc/slab_columns.hpp.  The
declarations of the five entry points in kernels.hpp are, byte for byte, what engine.hpp / psmatrix.cpp and the C ABI were
written against, and the three chain kernels are still __global__ definitions under the names that DESIGN.md, profiles/README.md
and kernel-trace filters use."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntpoly_amd", "csrc")

DECLARATIONS = [
    "bool slab_pade_chain(const DevMat& Base, const DevMat* const* addends, int n_addends, const double scales[2], const double* coeffs, DevMat& Out1,\n"
    "                     DevMat& Out2);\n",
    "bool slab_sum_chain(const DevMat& Base, double s, const DevMat* const* addends, const double* coeffs, int n_addends, double post, DevMat& Out);\n",
    "bool slab_poly_step(const DevMat& P, const DevMat& Q, const DevMat& R, double a, double c, DevMat& Tk, DevMat& Rout);\n",
    "bool slab_purify_tail(const DevMat& D, const DevMat& N, const DevMat& S, bool fold, DevMat& Out, double* norm, double dot[2]);\n",
    "bool slab_wom_heun(const DevMat& W, const DevMat& K0, const DevMat& K1, const DevMat& RK1, double h, double thr, DevMat& Out, double* err,\n"
    "                   double* err2);\n",
]
KERNELS = [("pade_chain.hip", "k_pade_chain"), ("sum_chain.hip", "k_sum_chain"), ("poly_step.hip", "k_poly_step")]


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


@pytest.mark.parametrize("decl", DECLARATIONS, ids=lambda d: d.split("(")[0].split()[-1])
def test_entry_point_declaration_is_unchanged(decl):
    assert _read("kernels.hpp").count("\n" + decl) == 1


@pytest.mark.parametrize("source,kernel", KERNELS)
def test_chain_kernel_is_defined_under_its_name(source, kernel):
    assert len(re.findall(r"__global__\s+__launch_bounds__\(256\)\s+void\s+%s\(" % kernel, _read(source))) == 1
