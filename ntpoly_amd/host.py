"""Python mirror of the reference's C++/SWIG classes (Source/CPlusPlus/*.h, the objects its own
unit tests use: ProcessGrid, TripletList_r/_c, Matrix_ps, Matrix_lsr/_lsc, MatrixMemoryPool,
Permutation, SolverParameters, DensityMatrixSolvers, SignSolvers, InverseSolvers,
SquareRootSolvers, LoadBalancer, EigenBounds) on top of the C ABI of libntpoly_amd.so.

Same method names and argument meaning as the reference so that the parity tests read like
the reference's tests.  numpy arrays are only used at the boundary (triplets in / out); all
matrix data lives in HBM.
"""
import contextlib
import ctypes as C

import numpy as np

from . import capi
from .capi import b, d, handle, i, lib, ll, s


# ------------------------------------------------------------------ process grid
def ConstructGlobalProcessGrid(process_rows=None, process_columns=None, process_slices=None, world_comm=0):
    """ProcessGrid.cc:12-48 (ConstructGlobalProcessGrid overloads)."""
    if process_rows is None and process_slices is None:
        lib.ConstructGlobalProcessGrid_default_wrp(i(world_comm))
    elif process_rows is None:
        lib.ConstructGlobalProcessGrid_onlyslice_wrp(i(world_comm), i(process_slices))
    else:
        lib.ConstructGlobalProcessGrid_wrp(i(world_comm), i(process_rows), i(process_columns), i(process_slices))


def WriteGridInfo():
    lib.WriteGlobalProcessGridInfo_wrp()


def DestructGlobalProcessGrid():
    lib.DestructGlobalProcessGrid_wrp()


def GetGlobalIsRoot():
    return bool(lib.GetGlobalIsRoot_wrp())


def init_comm(unique_id=None, rank=0, nranks=1):
    """RCCL bootstrap (replaces MPI_Init + communicator handles of the reference)."""
    if nranks <= 1:
        lib.ntpoly_amd_init_comm(b"\0" * 128, i(0), i(1))
    else:
        lib.ntpoly_amd_init_comm(unique_id, i(rank), i(nranks))


def get_unique_id():
    buf = C.create_string_buffer(128)
    lib.ntpoly_amd_get_unique_id(buf)
    return buf.raw


def init_comm_from_torch():
    """One process per GPU under torch.distributed.run: the 128-byte RCCL id is broadcast over a
    torch.distributed *gloo* group (control plane only) and the engine builds its own RCCL
    communicator (data plane, xGMI).  torch's GPU runtime is never initialised: the PyTorch wheel
    bundles a second HIP/RCCL runtime and two initialised runtimes in one process corrupt the heap
    at exit.  The engine picks its GPU from LOCAL_RANK.  Returns (rank, world_size)."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world <= 1:
        init_comm()
        return 0, 1
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("gloo")
    box = [get_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    init_comm(box[0], rank, world)
    return rank, world


def init_comm_from_env(timeout=300.0):
    """One process per GPU under `python -m torch.distributed.run` (or any launcher that sets RANK, WORLD_SIZE,
    LOCAL_RANK, MASTER_PORT) on ONE node, without importing torch: rank 0 creates the 128-byte RCCL id and hands
    it to the other ranks through a file in /tmp named after the launcher's pid (all ranks are children of the
    same launcher) and the master port; the engine then builds its own RCCL communicator and picks its GPU from
    LOCAL_RANK.  Returns (rank, world_size)."""
    import os
    import time
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world <= 1:
        init_comm()
        return 0, 1
    if os.environ.get("NTPOLY_AMD_COMM", "").startswith("shm:"):
        # shared-memory test transport: the segment name is in the environment, there is no id to hand over
        init_comm(get_unique_id(), rank, world)
        barrier()
        return rank, world
    # NTPOLY_AMD_RDV names the file explicitly (launchers whose ranks are not children of one process)
    path = os.environ.get("NTPOLY_AMD_RDV") or "/tmp/ntpoly_amd_rdv_%d_%s" % (os.getppid(), os.environ.get("MASTER_PORT", "0"))
    # a per-launch nonce keeps a stale file of an earlier (crashed) launch from being taken for this one's id
    # (an explicitly named file may be shared by ranks of different parents: NTPOLY_AMD_RDV_NONCE stands in for the pid)
    who = os.environ.get("NTPOLY_AMD_RDV_NONCE", "") if os.environ.get("NTPOLY_AMD_RDV") else str(os.getppid())
    # (an elastic restart of a crashed worker group keeps run id, port and parent: the restart count tells the new
    # group's file from the dead group's)
    # (hashed, not truncated: a long user-supplied run id must not push the restart count, port and parent out of the field)
    import hashlib
    nonce = hashlib.sha256((os.environ.get("TORCHELASTIC_RUN_ID", "") + ":" + os.environ.get("TORCHELASTIC_RESTART_COUNT", "0") + ":" +
                            os.environ.get("MASTER_PORT", "0") + ":" + who).encode()).hexdigest().encode()[:64].ljust(64, b"\0")
    if rank == 0:
        uid = get_unique_id()
        try:
            os.unlink(path)          # left behind by a launch that died between writing and joining
        except FileNotFoundError:
            pass
        tmp = "%s.%d.tmp" % (path, os.getpid())
        fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_EXCL | getattr(os, "O_NOFOLLOW", 0), 0o600)
        with os.fdopen(fd, "wb") as f:
            f.write(nonce + uid)
        os.rename(tmp, path)
    else:
        t0 = time.time()
        uid = None
        while uid is None:
            try:
                with open(path, "rb") as f:
                    blob = f.read()
                if len(blob) == 64 + 128 and blob[:64] == nonce:
                    uid = blob[64:]
            except FileNotFoundError:
                pass
            if uid is None:
                if time.time() - t0 > timeout:
                    raise RuntimeError("rendezvous file %s did not appear (or belongs to another launch)" % path)
                time.sleep(0.01)
    init_comm(uid, rank, world)
    barrier()
    if rank == 0:
        os.unlink(path)
    return rank, world


def barrier():
    lib.ntpoly_amd_barrier()


def allreduce_max(x):
    v = C.c_double(float(x))
    lib.ntpoly_amd_allreduce_max(C.byref(v), i(1))
    return v.value


def set_option(name, value):
    lib.ntpoly_amd_set_option(name.encode(), i(value))


def get_option(name):
    lib.ntpoly_amd_get_option.restype = C.c_int
    return int(lib.ntpoly_amd_get_option(name.encode()))


def synchronize():
    lib.ntpoly_amd_synchronize()


# ------------------------------------------------------------------ triplets
class Triplet_r:
    """Triplet.h: (index_column, index_row, point_value), 1-based indices"""
    def __init__(self, index_column=0, index_row=0, point_value=0.0):
        self.index_column, self.index_row, self.point_value = index_column, index_row, point_value

    def __iter__(self):
        return iter((self.index_column, self.index_row, self.point_value))


class Triplet_c(Triplet_r):
    pass


class _TripletList:
    _c = False

    def __init__(self, size=0):
        self.ih = handle()
        getattr(lib, "ConstructTripletList_%s_wrp" % self._sfx)(self.ih, i(size))

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            getattr(lib, "DestructTripletList_%s_wrp" % self._sfx)(self.ih)
            self.ih = None

    def GetSize(self):
        return int(getattr(lib, "GetTripletListSize_%s_wrp" % self._sfx)(self.ih))

    def Append(self, index_column, index_row=None, point_value=None):
        """Append(triplet) as the reference's SWIG classes take it (a Triplet_r / Triplet_c object), or the three
        fields directly"""
        if index_row is None:
            t = index_column
            index_column, index_row, point_value = t.index_column, t.index_row, t.point_value
        if self._c:
            lib.AppendToTripletList_c_wrp(self.ih, i(index_column), i(index_row), d(point_value.real), d(point_value.imag))
        else:
            lib.AppendToTripletList_r_wrp(self.ih, i(index_column), i(index_row), d(point_value))

    def GetTripletAt(self, index):
        """0-based index, as the reference's C++ / SWIG layer; returns a Triplet object that also unpacks as
        (index_column, index_row, point_value)"""
        col, row = C.c_int(), C.c_int()
        if self._c:
            re, im = C.c_double(), C.c_double()
            lib.GetTripletAt_c_wrp(self.ih, i(index + 1), C.byref(col), C.byref(row), C.byref(re), C.byref(im))
            return Triplet_c(col.value, row.value, complex(re.value, im.value))
        val = C.c_double()
        lib.GetTripletAt_r_wrp(self.ih, i(index + 1), C.byref(col), C.byref(row), C.byref(val))
        return Triplet_r(col.value, row.value, val.value)

    # bulk transfer (extension; the reference ABI moves one triplet per call)
    def set_arrays(self, col, row, val):
        col = np.ascontiguousarray(col, dtype=np.int32)
        row = np.ascontiguousarray(row, dtype=np.int32)
        if self._c:
            val = np.ascontiguousarray(val, dtype=np.complex128)
            lib.ntpoly_amd_triplets_set_c(self.ih, ll(len(col)), col.ctypes.data_as(C.c_void_p),
                                          row.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p))
        else:
            val = np.ascontiguousarray(val, dtype=np.float64)
            lib.ntpoly_amd_triplets_set_r(self.ih, ll(len(col)), col.ctypes.data_as(C.c_void_p),
                                          row.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p))

    def arrays(self):
        n = self.GetSize()
        col = np.empty(n, dtype=np.int32)
        row = np.empty(n, dtype=np.int32)
        val = np.empty(n, dtype=np.complex128 if self._c else np.float64)
        lib.ntpoly_amd_triplets_get(self.ih, col.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p),
                                    val.ctypes.data_as(C.c_void_p))
        return col, row, val


class TripletList_r(_TripletList):
    _sfx, _c = "r", False


class TripletList_c(_TripletList):
    _sfx, _c = "c", True


def _tlist_from(col, row, val):
    t = TripletList_c() if np.iscomplexobj(val) else TripletList_r()
    t.set_arrays(col, row, val)
    return t


# ------------------------------------------------------------------ permutation / parameters / pools
class Permutation:
    def __init__(self, matrix_dimension):
        self.ih = handle()
        self.dim = matrix_dimension
        lib.ConstructDefaultPermutation_wrp(self.ih, i(matrix_dimension))

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            lib.DestructPermutation_wrp(self.ih)
            self.ih = None

    def _rebuild(self, fn):
        lib.DestructPermutation_wrp(self.ih)
        getattr(lib, fn)(self.ih, i(self.dim))

    def SetDefaultPermutation(self):
        self._rebuild("ConstructDefaultPermutation_wrp")

    def SetReversePermutation(self):
        self._rebuild("ConstructReversePermutation_wrp")

    def SetRandomPermutation(self):
        self._rebuild("ConstructRandomPermutation_wrp")

    def set_lookup(self, index_lookup):
        arr = np.ascontiguousarray(index_lookup, dtype=np.int32)
        lib.ntpoly_amd_permutation_set(self.ih, i(len(arr)), arr.ctypes.data_as(C.c_void_p))


class SolverParameters:
    def __init__(self):
        self.ih = handle()
        lib.ConstructSolverParameters_wrp(self.ih)
        self._perm = None

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            lib.DestructSolverParameters_wrp(self.ih)
            self.ih = None

    def SetConvergeDiff(self, v):
        lib.SetParametersConvergeDiff_wrp(self.ih, d(v))

    def SetMaxIterations(self, v):
        lib.SetParametersMaxIterations_wrp(self.ih, i(v))

    def SetVerbosity(self, v):
        lib.SetParametersBeVerbose_wrp(self.ih, b(v))

    def SetThreshold(self, v):
        lib.SetParametersThreshold_wrp(self.ih, d(v))

    def SetLoadBalance(self, permutation):
        self._perm = permutation
        lib.SetParametersLoadBalance_wrp(self.ih, permutation.ih)

    def SetStepThreshold(self, v):
        lib.SetParametersStepThreshold_wrp(self.ih, d(v))

    def SetMonitorConvergence(self, v):
        lib.SetParametersMonitorConvergence_wrp(self.ih, b(v))


class PMatrixMemoryPool:
    def __init__(self, matrix):
        self.ih = handle()
        lib.ConstructMatrixMemoryPool_p_wrp(self.ih, matrix.ih)

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            lib.DestructMatrixMemoryPool_p_wrp(self.ih)
            self.ih = None


class MatrixMemoryPool_r:
    def __init__(self, columns, rows):
        self.ih = handle()
        lib.ConstructMatrixMemoryPool_lr_wrp(self.ih, i(columns), i(rows))

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            lib.DestructMatrixMemoryPool_lr_wrp(self.ih)
            self.ih = None


class MatrixMemoryPool_c(MatrixMemoryPool_r):
    def __init__(self, columns, rows):
        self.ih = handle()
        lib.ConstructMatrixMemoryPool_lc_wrp(self.ih, i(columns), i(rows))

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            lib.DestructMatrixMemoryPool_lc_wrp(self.ih)
            self.ih = None


# ------------------------------------------------------------------ distributed matrix
class Matrix_ps:
    """PSMatrix.h:20-197."""

    def __init__(self, arg=None):
        self.ih = handle()
        if isinstance(arg, Matrix_ps):
            lib.ConstructEmptyMatrix_ps_wrp(self.ih, i(arg.GetActualDimension()))
            lib.CopyMatrix_ps_wrp(arg.ih, self.ih)
        elif isinstance(arg, str):
            raw, n = s(arg)
            if arg.endswith(".mtx"):
                lib.ConstructMatrixFromMatrixMarket_ps_wrp(self.ih, raw, n)
            else:
                lib.ConstructMatrixFromBinary_ps_wrp(self.ih, raw, n)
        else:
            lib.ConstructEmptyMatrix_ps_wrp(self.ih, i(arg))

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            lib.DestructMatrix_ps_wrp(self.ih)
            self.ih = None

    # -- construction helpers used by the tests
    @classmethod
    def from_triplets(cls, dim, col, row, val):
        m = cls(dim)
        m.FillFromTripletList(_tlist_from(col, row, val))
        return m

    @classmethod
    def from_scipy(cls, mat):
        c = mat.tocsc()
        c.sort_indices()
        col = np.repeat(np.arange(c.shape[1], dtype=np.int32), np.diff(c.indptr)) + 1
        return cls.from_triplets(c.shape[0], col, c.indices.astype(np.int32) + 1, c.data)

    def triplets(self):
        """local triplets (col,row,val), 1-based global indices, sorted by column then row"""
        t = TripletList_c() if self.IsComplex() else TripletList_r()
        self.GetTripletList(t)
        return t.arrays()

    def to_scipy(self):
        import scipy.sparse as sp
        col, row, val = self.triplets()
        n = self.GetActualDimension()
        return sp.csc_matrix((val, (row - 1, col - 1)), shape=(n, n))

    # -- reference API
    def WriteToBinary(self, path):
        raw, n = s(path)
        lib.WriteMatrixToBinary_ps_wrp(self.ih, raw, n)

    def WriteToMatrixMarket(self, path):
        raw, n = s(path)
        lib.WriteMatrixToMatrixMarket_ps_wrp(self.ih, raw, n)

    def FillFromTripletList(self, tlist, prepartitioned=False):
        if prepartitioned:  # Fortran API: prepartitioned_in=.TRUE. (each rank passes its own columns)
            lib.ntpoly_amd_fill_prepartitioned(self.ih, tlist.ih)
        elif tlist._c:
            lib.FillMatrixFromTripletList_psc_wrp(self.ih, tlist.ih)
        else:
            lib.FillMatrixFromTripletList_psr_wrp(self.ih, tlist.ih)

    def FillPermutation(self, permutation, permuterows=True):
        lib.FillMatrixPermutation_ps_wrp(self.ih, permutation.ih, b(permuterows))

    def FillIdentity(self):
        lib.FillMatrixIdentity_ps_wrp(self.ih)

    def GetActualDimension(self):
        v = C.c_int()
        lib.GetMatrixActualDimension_ps_wrp(self.ih, C.byref(v))
        return v.value

    def GetLogicalDimension(self):
        v = C.c_int()
        lib.GetMatrixLogicalDimension_ps_wrp(self.ih, C.byref(v))
        return v.value

    def GetSize(self):
        v = C.c_long()
        lib.GetMatrixSize_ps_wrp(self.ih, C.byref(v))
        return v.value

    def IsComplex(self):
        return bool(lib.ntpoly_amd_matrix_is_complex(self.ih))

    def local_columns(self):
        a, c = C.c_int(), C.c_int()
        lib.ntpoly_amd_matrix_local_columns(self.ih, C.byref(a), C.byref(c))
        return a.value, c.value

    def GetTripletList(self, tlist):
        if tlist._c:
            lib.GetMatrixTripletList_psc_wrp(self.ih, tlist.ih)
        else:
            lib.GetMatrixTripletList_psr_wrp(self.ih, tlist.ih)

    def Transpose(self, matA):
        lib.TransposeMatrix_ps_wrp(matA.ih, self.ih)

    def Conjugate(self):
        lib.ConjugateMatrix_ps_wrp(self.ih)

    def Dot(self, matB):
        if self.IsComplex() or matB.IsComplex():
            re, im = C.c_double(), C.c_double()
            lib.DotMatrix_psc_wrp(self.ih, matB.ih, C.byref(re), C.byref(im))
            return complex(re.value, im.value)
        v = C.c_double()
        lib.DotMatrix_psr_wrp(self.ih, matB.ih, C.byref(v))
        return v.value

    def Increment(self, matB, alpha=1.0, threshold=0.0):
        """this <- alpha*matB + this (PSMatrix.cc Increment)"""
        lib.IncrementMatrix_ps_wrp(matB.ih, self.ih, d(alpha), d(threshold))

    def PairwiseMultiply(self, matA, matB):
        lib.MatrixPairwiseMultiply_ps_wrp(matA.ih, matB.ih, self.ih)

    def Gemm(self, matA, matB, memory_pool=None, alpha=1.0, beta=0.0, threshold=0.0):
        """this = alpha*matA*matB + beta*this (PSMatrix.cc:208-213)"""
        pool = memory_pool if memory_pool is not None else PMatrixMemoryPool(matA)
        lib.MatrixMultiply_ps_wrp(matA.ih, matB.ih, self.ih, d(alpha), d(beta), d(threshold), pool.ih)

    def Scale(self, constant):
        lib.ScaleMatrix_ps_wrp(self.ih, d(constant))

    def Norm(self):
        return float(lib.MatrixNorm_ps_wrp(self.ih))

    def MeasureAsymmetry(self):
        return float(lib.MeasureAsymmetry_ps_wrp(self.ih))

    def Trace(self):
        v = C.c_double()
        lib.MatrixTrace_ps_wrp(self.ih, C.byref(v))
        return v.value

    def IsIdentity(self):
        return bool(lib.IsIdentity_ps_wrp(self.ih))

    def Symmetrize(self):
        lib.SymmetrizeMatrix_ps_wrp(self.ih)

    def CommSplit(self):
        """(copy of the WHOLE matrix on this process's half of the grid, colour 0 / 1, True when the grid was split along its
        slices) -- CommSplitMatrix, PSMatrixModule.F90:1489-1541; the copy lives on a sub-communicator: everything done with
        it afterwards (products, reductions, solvers) stays inside the half"""
        out = Matrix_ps.__new__(Matrix_ps)
        out.ih = handle()
        color = C.c_int(0)
        split_slice = C.c_bool(False)
        lib.ntpoly_amd_comm_split_matrix(self.ih, out.ih, C.byref(color), C.byref(split_slice))
        return out, int(color.value), bool(split_slice.value)

    def grid_comm_info(self):
        """(rank on the communicator of this matrix's grid, its size, True when that is a sub-communicator)"""
        g = handle()
        lib.GetMatrixProcessGrid_ps_wrp(self.ih, g)
        out = (C.c_int * 3)()
        lib.ntpoly_amd_grid_comm_info(g, out)
        return int(out[0]), int(out[1]), bool(out[2])

    def GatherMatrixToProcess(self, within_slice_id=None):
        """the whole matrix as a LOCAL matrix on every process (None) or on the process with this rank inside its slice (the
        others get None) -- PSMatrixModule.F90:1704-1808"""
        cls = Matrix_lsc if self.IsComplex() else Matrix_lsr
        ih = handle()
        lib.ntpoly_amd_gather_matrix_to_process(self.ih, ih, i(-1 if within_slice_id is None else within_slice_id))
        if not any(ih):
            return None
        out = cls.__new__(cls)
        out.ih = ih
        return out


# ------------------------------------------------------------------ local matrices (config 2)
class _Matrix_ls:
    def __init__(self, rows=None, columns=None, tlist=None, path=None):
        self.ih = handle()
        sfx = self._sfx
        if path is not None:
            raw, n = s(path)
            getattr(lib, "ConstructMatrixFromFile_%s_wrp" % sfx)(self.ih, raw, n)
        elif tlist is not None:
            getattr(lib, "ConstructMatrixFromTripletList_%s_wrp" % sfx)(self.ih, tlist.ih, i(rows), i(columns))
        else:
            getattr(lib, "ConstructZeroMatrix_%s_wrp" % sfx)(self.ih, i(rows), i(columns))

    def __del__(self):
        if getattr(self, "ih", None) is not None and lib is not None:
            getattr(lib, "DestructMatrix_%s_wrp" % self._sfx)(self.ih)
            self.ih = None

    @classmethod
    def from_triplets(cls, rows, cols, col, row, val):
        return cls(rows, cols, tlist=_tlist_from(col, row, val))

    def GetRows(self):
        v = C.c_int()
        getattr(lib, "GetMatrixRows_%s_wrp" % self._sfx)(self.ih, C.byref(v))
        return v.value

    def GetColumns(self):
        v = C.c_int()
        getattr(lib, "GetMatrixColumns_%s_wrp" % self._sfx)(self.ih, C.byref(v))
        return v.value

    def Scale(self, c):
        getattr(lib, "ScaleMatrix_%s_wrp" % self._sfx)(self.ih, d(c))

    def Increment(self, matB, alpha=1.0, threshold=0.0):
        getattr(lib, "IncrementMatrix_%s_wrp" % self._sfx)(matB.ih, self.ih, d(alpha), d(threshold))

    def PairwiseMultiply(self, matA, matB):
        getattr(lib, "PairwiseMultiplyMatrix_%s_wrp" % self._sfx)(matA.ih, matB.ih, self.ih)

    def Gemm(self, matA, matB, isATransposed=False, isBTransposed=False, alpha=1.0, beta=0.0, threshold=0.0,
             memory_pool=None):
        """this = alpha*op(matA)*op(matB) + beta*this (SMatrix.cc Gemm)"""
        pool = memory_pool if memory_pool is not None else self._pool(matB.GetColumns(), matA.GetRows())
        getattr(lib, "MatrixMultiply_%s_wrp" % self._sfx)(matA.ih, matB.ih, self.ih, b(isATransposed), b(isBTransposed),
                                                          d(alpha), d(beta), d(threshold), pool.ih)

    def Transpose(self, matA):
        getattr(lib, "TransposeMatrix_%s_wrp" % self._sfx)(matA.ih, self.ih)

    def triplets(self):
        t = TripletList_c() if self._sfx == "lsc" else TripletList_r()
        getattr(lib, "MatrixToTripletList_%s_wrp" % self._sfx)(self.ih, t.ih)
        return t.arrays()


class Matrix_lsr(_Matrix_ls):
    _sfx, _pool = "lsr", MatrixMemoryPool_r

    def Dot(self, matB):
        v = C.c_double()
        lib.DotMatrix_lsr_wrp(self.ih, matB.ih, C.byref(v))
        return v.value


class Matrix_lsc(_Matrix_ls):
    _sfx, _pool = "lsc", MatrixMemoryPool_c

    def Dot(self, matB):
        re, im = C.c_double(), C.c_double()
        lib.DotMatrix_lsc_wrp(self.ih, matB.ih, C.byref(re), C.byref(im))
        return complex(re.value, im.value)

    def Conjugate(self):
        lib.ConjugateMatrix_lsc_wrp(self.ih)


# ------------------------------------------------------------------ solvers (static-method classes as in Source/CPlusPlus)
class DensityMatrixSolvers:
    @staticmethod
    def _run(fn, Hamiltonian, InverseSquareRoot, trace, Density, solver_parameters):
        e, mu = C.c_double(), C.c_double()
        fn(Hamiltonian.ih, InverseSquareRoot.ih, d(trace), Density.ih, C.byref(e), C.byref(mu), solver_parameters.ih)
        return e.value, mu.value

    @staticmethod
    def PM(H, ISQ, trace, Density, solver_parameters):
        return DensityMatrixSolvers._run(lib.PM_wrp, H, ISQ, trace, Density, solver_parameters)

    @staticmethod
    def TRS2(H, ISQ, trace, Density, solver_parameters):
        return DensityMatrixSolvers._run(lib.TRS2_wrp, H, ISQ, trace, Density, solver_parameters)

    @staticmethod
    def TRS4(H, ISQ, trace, Density, solver_parameters):
        return DensityMatrixSolvers._run(lib.TRS4_wrp, H, ISQ, trace, Density, solver_parameters)

    @staticmethod
    def HPCP(H, ISQ, trace, Density, solver_parameters):
        return DensityMatrixSolvers._run(lib.HPCP_wrp, H, ISQ, trace, Density, solver_parameters)

    @staticmethod
    def ScaleAndFold(H, ISQ, trace, Density, homo, lumo, solver_parameters):
        """rubensson2011nonmonotonic; homo / lumo: conservative estimates of the highest occupied and the lowest unoccupied
        eigenvalue.  Returns the energy (the method computes no chemical potential)."""
        e = C.c_double()
        lib.ScaleAndFold_wrp(H.ih, ISQ.ih, d(trace), Density.ih, d(homo), d(lumo), C.byref(e), solver_parameters.ih)
        return e.value


def trs2_step(X, X2, WH, trace, threshold, trace_x=None):
    """one TRS2 iteration (what TRS2_wrp runs inside its loop) -> (sigma, energy, trace of the new X);
    trace_x = trace of X from the previous step's return value (None: computed).  X2 is SCRATCH: on the fused path the
    product X*X never exists as a matrix (it is merged into X inside the SpGEMM kernel's epilogue) and X2 is left
    untouched; only the unfused path leaves X*X in it."""
    e, sg = C.c_double(), C.c_double()
    tr = C.c_double(float("nan") if trace_x is None else trace_x)
    lib.ntpoly_amd_trs2_step(X.ih, X2.ih, WH.ih, d(trace), d(threshold), C.byref(e), C.byref(sg), C.byref(tr))
    return sg.value, e.value, tr.value


class SignSolvers:
    @staticmethod
    def ComputeSign(mat, signmat, solver_parameters):
        lib.SignFunction_wrp(mat.ih, signmat.ih, solver_parameters.ih)

    @staticmethod
    def ComputePolarDecomposition(mat, umat, hmat, solver_parameters):
        lib.PolarDecomposition_wrp(mat.ih, umat.ih, hmat.ih, solver_parameters.ih)


class InverseSolvers:
    @staticmethod
    def Invert(mat, inverse, solver_parameters):
        lib.Invert_wrp(mat.ih, inverse.ih, solver_parameters.ih)

    @staticmethod
    def PseudoInverse(mat, inverse, solver_parameters):
        lib.PseudoInverse_wrp(mat.ih, inverse.ih, solver_parameters.ih)


class SquareRootSolvers:
    @staticmethod
    def SquareRoot(mat, out, solver_parameters):
        lib.SquareRoot_wrp(mat.ih, out.ih, solver_parameters.ih)

    @staticmethod
    def InverseSquareRoot(mat, out, solver_parameters):
        lib.InverseSquareRoot_wrp(mat.ih, out.ih, solver_parameters.ih)

    @staticmethod
    def with_order(mat, out, solver_parameters, inverse, order):
        lib.ntpoly_amd_square_root_order(mat.ih, out.ih, solver_parameters.ih, i(int(inverse)), i(order))


class _Poly:
    """Polynomial.h / ChebyshevSolvers.h / HermiteSolvers.h: coefficient `degree` (0-based) multiplies
    x^degree, T_degree(x) or H_degree(x)"""
    _construct = _destruct = _set = None

    def __init__(self, degree):
        self.ih = handle()
        getattr(lib, self._construct)(self.ih, i(degree))

    def __del__(self):
        try:
            getattr(lib, self._destruct)(self.ih)
        except Exception:
            pass

    def SetCoefficient(self, degree, coefficient):
        getattr(lib, self._set)(self.ih, i(degree + 1), d(coefficient))


class Polynomial(_Poly):
    _construct, _destruct, _set = "ConstructPolynomial_wrp", "DestructPolynomial_wrp", "SetCoefficient_wrp"

    def HornerCompute(self, InputMat, OutputMat, solver_parameters):
        lib.HornerCompute_wrp(InputMat.ih, OutputMat.ih, self.ih, solver_parameters.ih)

    def PatersonStockmeyerCompute(self, InputMat, OutputMat, solver_parameters):
        lib.PatersonStockmeyerCompute_wrp(InputMat.ih, OutputMat.ih, self.ih, solver_parameters.ih)


class ChebyshevPolynomial(_Poly):
    _construct, _destruct, _set = ("ConstructChebyshevPolynomial_wrp", "DestructChebyshevPolynomial_wrp",
                                   "SetChebyshevCoefficient_wrp")

    def Compute(self, InputMat, OutputMat, solver_parameters):
        lib.ChebyshevCompute_wrp(InputMat.ih, OutputMat.ih, self.ih, solver_parameters.ih)

    def ComputeFactorized(self, InputMat, OutputMat, solver_parameters):
        lib.FactorizedChebyshevCompute_wrp(InputMat.ih, OutputMat.ih, self.ih, solver_parameters.ih)


class HermitePolynomial(_Poly):
    _construct, _destruct, _set = ("ConstructHermitePolynomial_wrp", "DestructHermitePolynomial_wrp",
                                   "SetHermiteCoefficient_wrp")

    def Compute(self, InputMat, OutputMat, solver_parameters):
        lib.HermiteCompute_wrp(InputMat.ih, OutputMat.ih, self.ih, solver_parameters.ih)


class ExponentialSolvers:
    @staticmethod
    def ComputeExponential(InputMat, OutputMat, solver_parameters):
        lib.ComputeExponential_wrp(InputMat.ih, OutputMat.ih, solver_parameters.ih)

    @staticmethod
    def ComputeLogarithm(InputMat, OutputMat, solver_parameters):
        lib.ComputeLogarithm_wrp(InputMat.ih, OutputMat.ih, solver_parameters.ih)

    @staticmethod
    def ComputeExponentialPade(InputMat, OutputMat, solver_parameters):
        lib.ComputeExponentialPade_wrp(InputMat.ih, OutputMat.ih, solver_parameters.ih)


class TrigonometrySolvers:
    @staticmethod
    def Sine(InputMat, OutputMat, solver_parameters):
        lib.Sine_wrp(InputMat.ih, OutputMat.ih, solver_parameters.ih)

    @staticmethod
    def Cosine(InputMat, OutputMat, solver_parameters):
        lib.Cosine_wrp(InputMat.ih, OutputMat.ih, solver_parameters.ih)


class RootSolvers:
    @staticmethod
    def ComputeRoot(InputMat, OutputMat, root, solver_parameters):
        lib.ComputeRoot_wrp(InputMat.ih, OutputMat.ih, i(root), solver_parameters.ih)

    @staticmethod
    def ComputeInverseRoot(InputMat, OutputMat, root, solver_parameters):
        lib.ComputeInverseRoot_wrp(InputMat.ih, OutputMat.ih, i(root), solver_parameters.ih)


class LinearSolvers:
    """Source/CPlusPlus/LinearSolvers.h"""
    @staticmethod
    def CGSolver(AMat, XMat, BMat, solver_parameters):
        lib.CGSolver_wrp(AMat.ih, XMat.ih, BMat.ih, solver_parameters.ih)

    @staticmethod
    def CholeskyDecomposition(AMat, LMat, solver_parameters):
        lib.CholeskyDecomposition_wrp(AMat.ih, LMat.ih, solver_parameters.ih)


class Analysis:
    """Source/CPlusPlus/Analysis.h"""
    @staticmethod
    def PivotedCholeskyDecomposition(AMat, LMat, rank, solver_parameters):
        lib.PivotedCholeskyDecomposition_wrp(AMat.ih, LMat.ih, i(rank), solver_parameters.ih)

    @staticmethod
    def ReduceDimension(AMat, dim, RMat, solver_parameters):
        lib.ReduceDimension_wrp(AMat.ih, i(dim), RMat.ih, solver_parameters.ih)


class GeometryOptimization:
    """Source/CPlusPlus/GeometryOptimization.h"""
    @staticmethod
    def PurificationExtrapolate(PreviousDensity, Overlap, trace, NewDensity, solver_parameters):
        lib.PurificationExtrapolate_wrp(PreviousDensity.ih, Overlap.ih, d(trace), NewDensity.ih, solver_parameters.ih)

    @staticmethod
    def LowdinExtrapolate(PreviousDensity, OldOverlap, NewOverlap, NewDensity, solver_parameters):
        lib.LowdinExtrapolate_wrp(PreviousDensity.ih, OldOverlap.ih, NewOverlap.ih, NewDensity.ih, solver_parameters.ih)


class MatrixConversion:
    """Source/CPlusPlus/MatrixConversion.h"""
    @staticmethod
    def SnapMatrixToSparsityPattern(mat, pattern):
        lib.SnapMatrixToSparsityPattern_wrp(mat.ih, pattern.ih)


class EigenSolvers:
    """Source/CPlusPlus/EigenSolvers.h (the dense eigensolver is the engine's own Jacobi method on the GPU)"""
    @staticmethod
    def EigenDecomposition(matrix, eigenvalues, nvals, eigenvectors, solver_parameters):
        lib.EigenDecomposition_wrp(matrix.ih, eigenvalues.ih, i(nvals), eigenvectors.ih, solver_parameters.ih)

    @staticmethod
    def EigenValues(matrix, eigenvalues, nvals, solver_parameters):
        lib.EigenDecomposition_novec_wrp(matrix.ih, eigenvalues.ih, i(nvals), solver_parameters.ih)

    @staticmethod
    def SingularValueDecomposition(matrix, leftvectors, rightvectors, singularvalues, solver_parameters):
        lib.SingularValueDecompostion_wrp(matrix.ih, leftvectors.ih, rightvectors.ih, singularvalues.ih,
                                          solver_parameters.ih)

    @staticmethod
    def EstimateGap(H, K, chemical_potential, solver_parameters):
        gap = C.c_double()
        lib.EstimateGap_wrp(H.ih, K.ih, d(chemical_potential), C.byref(gap), solver_parameters.ih)
        return gap.value


class FermiOperator:
    """Source/CPlusPlus/FermiOperator.h; each returns (energy, chemical potential or None)"""
    @staticmethod
    def ComputeDenseFOE(H, ISQ, trace, Density, inv_temp, solver_parameters):
        e, mu = C.c_double(), C.c_double()
        lib.ComputeDenseFOE_wrp(H.ih, ISQ.ih, d(trace), Density.ih, d(inv_temp), C.byref(e), C.byref(mu), solver_parameters.ih)
        return e.value, mu.value

    @staticmethod
    def WOM_GC(H, ISQ, Density, chemical_potential, inv_temp, solver_parameters):
        e = C.c_double()
        lib.WOM_GC_wrp(H.ih, ISQ.ih, Density.ih, d(chemical_potential), d(inv_temp), C.byref(e), solver_parameters.ih)
        return e.value

    @staticmethod
    def WOM_C(H, ISQ, Density, trace, inv_temp, solver_parameters):
        e = C.c_double()
        lib.WOM_C_wrp(H.ih, ISQ.ih, Density.ih, d(trace), d(inv_temp), C.byref(e), solver_parameters.ih)
        return e.value


class DenseSolvers:
    """the reference's Dense* entry points (f(A) = V f(L) V^H through the eigendecomposition)"""
    @staticmethod
    def DenseDensity(H, ISQ, trace, Density, solver_parameters):
        return DensityMatrixSolvers._run(lib.DenseDensity_wrp, H, ISQ, trace, Density, solver_parameters)

    @staticmethod
    def _f(name, In, Out, solver_parameters):
        getattr(lib, name)(In.ih, Out.ih, solver_parameters.ih)

    SquareRoot = staticmethod(lambda a, o, p: DenseSolvers._f("DenseSquareRoot_wrp", a, o, p))
    InverseSquareRoot = staticmethod(lambda a, o, p: DenseSolvers._f("DenseInverseSquareRoot_wrp", a, o, p))
    Exponential = staticmethod(lambda a, o, p: DenseSolvers._f("ComputeDenseExponential_wrp", a, o, p))
    Logarithm = staticmethod(lambda a, o, p: DenseSolvers._f("ComputeDenseLogarithm_wrp", a, o, p))
    Sine = staticmethod(lambda a, o, p: DenseSolvers._f("DenseSine_wrp", a, o, p))
    Cosine = staticmethod(lambda a, o, p: DenseSolvers._f("DenseCosine_wrp", a, o, p))
    Invert = staticmethod(lambda a, o, p: DenseSolvers._f("DenseInvert_wrp", a, o, p))
    SignFunction = staticmethod(lambda a, o, p: DenseSolvers._f("DenseSignFunction_wrp", a, o, p))


class LoadBalancer:
    @staticmethod
    def PermuteMatrix(mat_in, mat_out, permutation, memorypool=None):
        pool = memorypool if memorypool is not None else PMatrixMemoryPool(mat_in)
        lib.PermuteMatrix_wrp(mat_in.ih, mat_out.ih, permutation.ih, pool.ih)

    @staticmethod
    def UndoPermuteMatrix(mat_in, mat_out, permutation, memorypool=None):
        pool = memorypool if memorypool is not None else PMatrixMemoryPool(mat_in)
        lib.UndoPermuteMatrix_wrp(mat_in.ih, mat_out.ih, permutation.ih, pool.ih)


class EigenBounds:
    @staticmethod
    def PowerBounds(matrix, solver_parameters):
        v = C.c_double()
        lib.PowerBounds_wrp(matrix.ih, C.byref(v), solver_parameters.ih)
        return v.value

    @staticmethod
    def GershgorinBounds(matrix):
        mn, mx = C.c_double(), C.c_double()
        lib.GershgorinBounds_wrp(matrix.ih, C.byref(mn), C.byref(mx))
        return mn.value, mx.value


def ActivateLogger(start_document=False, file_name=None):
    if file_name:
        raw, n = s(file_name)
        lib.ActivateLoggerFile_wrp(b(start_document), raw, n)
    else:
        lib.ActivateLogger_wrp(b(start_document))


def DeactivateLogger():
    lib.DeactivateLogger_wrp()


# ------------------------------------------------------------------ statistics (extensions)
def last_spgemm_stats():
    out = (C.c_longlong * 13)()
    a, t = C.c_float(), C.c_float()
    lib.ntpoly_amd_last_spgemm_stats(out, C.byref(a), C.byref(t))
    return dict(nnz_a=out[0], nnz_b=out[1], nnz_c=out[2], products=out[3], tmp_entries=out[4],
                bins=[out[5 + k] for k in range(6)], overflow=out[11], slab=out[12], ms_numeric=a.value, ms_total=t.value)


def band_order(M):
    """(new position of every index, bandwidth) of the bandwidth-reducing order of M's pattern (csrc/relabel.hip), or None"""
    pos = np.zeros(M.GetActualDimension(), dtype=np.int32)
    bw = C.c_longlong()
    lib.ntpoly_amd_band_order.restype = C.c_int
    ok = lib.ntpoly_amd_band_order(M.ih, pos.ctypes.data_as(C.c_void_p), C.byref(bw))
    return (pos, int(bw.value)) if ok else None


# The counter arrays of csrc/counters.inc: name -> (keys of the slots in the table's order, docstring[, tuple]).  Every entry
# becomes <name>_counts(), which reads ntpoly_amd_<name>_counts and returns a dict under these keys (with `tuple`: the bare values).
_COUNTERS = {
    "fusion": (("square", "update", "repeated"),
               """(steps X*X, steps 2X - X*X) computed inside the SpGEMM kernel's epilogue and fused steps repeated unfused"""),
    "complex_fusion": (("square", "update", "repeated"),
                       """complex TRS2 steps X*X and 2X - X*X done in complex slab or block form (product, merge and energy pass -- not a fused
    tile epilogue), and such steps repeated the old way"""),
    "tile2": (("done", "repeated"),
              """(multiplies computed in the two-block geometry of the MFMA kernel, launches of it repeated on k_spgemm_tile)"""),
    "tile_skip": (("tested", "skipped"),
                  """(tiles the MFMA tile kernel tested against the operand's segment maxima, tiles it skipped) since reset_spgemm_accum""",
                  tuple),
    "band_scope": (("solves", "searched"),
                   """(solves run in a recovered band order across ranks, operands searched for a hidden band)"""),
    "slab_algebra": (("products", "merges", "others", "refusals"),
                     """operations of the solver loops done on matrices in slab form since start, and those that went back to compressed columns"""),
    "slab_view": (("built", "products", "taken", "declined"),
                  """read-only slab views of operands that store zeros (option stored_zero_views) since start: views built from compressed
    columns, products / merges-copies-scalings with a view operand done in slab form, merges on a view declined because the
    result would hold a stored zero"""),
    "ghash_class": (("real_mfma", "real_vector", "complex_mfma", "complex_vector"),
                    """groups finished by the grouped LDS-hash kernel (csrc/spgemm_grouped.hip) since start, by path: real operands on the matrix
    cores (option ghash_mfma) / on the vector units, complex operands on the matrix cores (option ghash_mfma_complex: table class 0
    in FMA arithmetic with complex_tile, two FMA chains per part of an entry) / on the vector units"""),
    "panel_product": (("slab", "declined", "host_syncs"),
                      """products of slab sessions on more than one rank since start: done in slab form on every rank, declined"""),
    "thin_slab": (("real_left", "real_right", "complex_left", "complex_right", "panel_real", "panel_complex"),
                  """products of slab sessions on the thin-operand gather kernels (csrc/spgemm_thin.hip) since start: real / complex, thin left /
    right operand; of those, the panel products (slab sessions on several ranks), real and complex"""),
    "pm_session": (("sigma", "updates", "zeros", "left"),
                   """PM purification on a slab-form iterate (option pm_session; csrc/slab_extra.hip) since start: sigma passes fused, updates fused,
    stored zeros carried beside the runs (summed over the updates), solves that left the fused path"""),
    "complex_pm": (("sigma", "updates", "zeros", "left"),
                   """complex PM in a complex slab session (option complex_pm; csrc/slab_extra.hip k_pm_sigma / k_pm_update on runs of (re, im)
    pairs) since start: sigma passes fused, updates fused, stored (0, 0) entries carried beside the runs (summed over the updates),
    solves that left the fused path; slab_algebra_counts() counts a fused pass as the real branch does.  A solve kept out by a gate
    (the option off, several ranks, iterates in block form) counts nowhere; real operands count in pm_session_counts() only"""),
    "isr_chain": (("order5", "order3", "refused"),
                  """the polynomial chain of the Taylor square-root step in one pass (option isr_chain; csrc/slab_extra.hip k_sa_isr_chain) since
    start: order-5 chains fused, order-3 chains fused, chains refused (the vocabulary calls ran instead); slab_algebra_counts()
    counts a fused chain as the four / two merges it replaces.  A step kept out by a gate (the option off, no session for the
    operands' kind, X and X X both in compressed columns, a labelled slab form) is neither fused nor counted as refused"""),
    "slab_transpose": (("transposes", "conjugates", "refused", "polar_sessions"),
                       """the transpose of a slab form (option slab_transpose; csrc/slab_extra.hip k_tr_extents / k_tr_values) since start: transposes
    done in slab form, conjugations done in slab form, transposes refused past the gates (extents far apart: that one ran on
    compressed columns), PolarDecomposition solves that ran in a slab session.  A gated operand (no session, several ranks,
    compressed columns, a view, a labelled form, block form) counts nowhere"""),
    "power_vector": (("solves", "steps", "refused"),
                     """PowerBounds on one vector (option power_vector; csrc/power_vector.hip) since start: solves that ran on one vector, power
    steps computed by k_pv_step, solves that passed the gates but were refused (the gather form could not be built: the N-column
    loop ran).  A solve kept out by a gate (the option off, process slices > 1) counts nowhere; power_vector_step() counts nothing"""),
    "cg_dots": (("solves", "passes", "refused", "not_formed"),
                """CGSolver with its traces from column dot passes (option cg_dots; csrc/cg_dots.hip k_cg_dots / k_cg_trace) since start: solves
    that ran with the passes, dot passes done by the kernel, passes refused past the gates (the same chains ran on the rank's
    compressed columns), products and transposes not formed.  A solve kept out by a gate (the option off, no session for the
    operands' kind, block form, process slices > 1, complex operands with the option below 2 or on several ranks) counts nowhere;
    cg_dots() counts nothing"""),
    "hpcp_step": (("traces", "updates", "refused"),
                  """HPCP purification with its traces and its update in one pass each (option hpcp_step; csrc/slab_extra.hip k_hpcp_traces /
    k_hpcp_update) since start: trace passes fused, updates fused, updates refused (the vocabulary calls ran instead);
    slab_algebra_counts() counts a fused update as the four merges / copies and the two other operations it replaces.  A step kept
    out by a gate (the option off, no open real session, a complex operand, block form, a labelled slab form, alignments that
    differ, a WH the dot cannot read as runs) is neither fused nor counted as refused"""),
    "complex_hpcp": (("traces", "updates", "refused"),
                     """complex HPCP in a complex slab session (option complex_hpcp; csrc/slab_extra.hip k_hpcp_traces / k_hpcp_update on runs of
    (re, im) pairs) since start: trace passes fused, updates fused, passes refused (the vocabulary calls ran instead);
    slab_algebra_counts() counts a fused pass as the real branch does.  A pass kept out by a gate (the option off, no open complex
    session, several ranks, block form, a labelled slab form, alignments that differ, a WH the dot cannot read as runs) is neither
    fused nor counted as refused; real operands count in hpcp_step_counts() only"""),
    "scale_fold_step": (("updates", "dot_traces", "refused"),
                        """ScaleAndFold with the update, the energy and the next step's trace in one pass (option scale_fold_step; csrc/slab_extra.hip
    k_saf_update / k_saf_dot_trace) since start: fold updates fused, dot-and-trace passes fused (the scale branch), passes refused
    (the vocabulary calls ran instead); slab_algebra_counts() counts a fused pass as the calls it replaces (the merge of an
    update, the dot, the next trace).  A step kept out by a gate (the option off, no open real session, a complex operand, block
    form, a labelled slab form, alignments that differ, a WH the dot cannot read as runs) is neither fused nor counted as refused"""),
    "wom_session": (("solves", "heun_passes", "c_dot_passes", "refused"),
                    """WOM_GC / WOM_C in a slab session (option wom_session; csrc/wom_heun.hip k_wom_heun / k_wom_c_dots) since start: solves that
    ran in a slab session, Heun tails fused, pairs of dots of the canonical step fused, passes refused past the gates (the vocabulary
    calls ran instead); slab_algebra_counts() counts a fused pass as the calls it replaces (seven merges / copies and two norms; two
    dots).  A pass kept out by a gate (the option below 2, no open real session, a complex operand, block form, a labelled slab
    form, dimensions that differ, one matrix given twice) counts nowhere"""),
    "purify_session": (("solves", "fold_passes", "plain_passes", "refused"),
                       """PurificationExtrapolate in a slab session (option purify_session; csrc/purify_tail.hip k_purify_tail) since start: solves
    that ran in a slab session, tails fused in the fold branch (N' = 2 D - D S D written), tails fused in the plain branch (nothing
    written), passes refused past the gates (the vocabulary calls ran instead); slab_algebra_counts() counts a fused pass as the
    calls it replaces (fold: two merges, the copy, the scaling, the norm and the dot; plain: one merge, the copy, the norm and the
    dot).  A pass kept out by a gate (the option below 2, no open real session, a complex operand, block form, a labelled slab
    form, dimensions that differ, one matrix given twice) counts nowhere"""),
    "pade_session": (("solves", "sum_passes", "pair_passes", "refused"),
                     """ComputeExponentialPade in a slab session (option pade_session; csrc/pade_chain.hip k_pade_chain) since start: calls that ran in
    a slab session, sum passes fused (P1 and TempMat from I, B1, B2, B3 in one pass), pair passes fused (LeftMat and RightMat from P1
    and P2 in one pass), passes refused past the gates (the vocabulary calls ran instead); slab_algebra_counts() counts a fused pass
    as the calls it replaces (two copies, the merges, the scalings).  A pass kept out by a gate (the option below 2, no open real
    session, a complex operand, block form, a labelled slab form, dimensions that differ, one matrix given twice, a number of
    addends other than 1 or 3) counts nowhere"""),
    "poly_step": (("exp_sessions", "steps", "refused"),
                  """the real Chebyshev / Hermite step in one pass and ComputeExponential's squarings in a slab session (option poly_step;
    csrc/poly_step.hip k_poly_step) since start: ComputeExponential calls whose real squarings ran in a slab session, steps fused
    (Tk = P + a T(k-2) and R += c Tk in one pass), passes refused past the gates (the two merges ran instead); slab_algebra_counts()
    counts a fused step as the two merges it replaces.  A step kept out by a gate (the option below 2, no open real session, a
    complex operand, block form, a labelled slab form, dimensions that differ, one matrix in two roles, a zero coefficient, a grid
    with process slices) counts nowhere"""),
    "sum_chain": (("passes", "refused"),
                  """the scaled sum chain of the real solver loops in one pass (option sum_chain; csrc/sum_chain.hip k_sum_chain) since start:
    passes fused (CopyMatrix, ScaleMatrix, up to five IncrementMatrix calls at threshold 0 and a trailing ScaleMatrix in one pass),
    passes refused past the gates (the vocabulary calls ran instead); slab_algebra_counts() counts a fused pass as the calls it
    replaces.  A pass kept out by a gate (the option at 0, no open real session, a complex operand, block form, a labelled slab
    form, dimensions that differ, one matrix in two input roles, the output among the addends, a number of addends outside 1 .. 5,
    a grid with process slices, a scalar that is zero or not finite) counts nowhere"""),
    "complex_sum_chain": (("sessions", "passes", "refused"),
                          """the complex side of the sum chain (option complex_sum_chain; csrc/sum_chain.hip k_sum_chain<double2, M>) since start:
    inverse-root loops that opened a complex slab session (level 1), passes fused (level 2: the chain on runs of (re, im) pairs in one
    pass), passes refused past the gates (the vocabulary calls ran instead); slab_algebra_counts() counts a fused pass as the real
    branch does.  A pass kept out by a gate (the option below 2, no open session that takes complex operands, block form, a labelled
    slab form, dimensions that differ, one matrix in two input roles, the output among the addends, a number of addends outside
    1 .. 5, a grid with process slices, real and complex operands mixed, a scalar that is zero or not finite) counts nowhere; real
    operands count in sum_chain_counts() only"""),
    "complex_scale_fold": (("updates", "dot_traces", "refused"),
                           """complex ScaleAndFold in a complex slab session (option complex_scale_fold; csrc/slab_extra.hip k_saf_update on runs of (re, im)
    pairs, k_sa_dot_trace_c for the scale branch) since start: fold updates fused, dot-and-trace passes fused, passes refused (the
    vocabulary calls ran instead); slab_algebra_counts() counts a fused pass as the real branch does.  A pass kept out by a gate (the
    option off, no open complex session, several ranks, block form, a labelled slab form, alignments that differ, a WH the dot
    cannot read) is neither fused nor counted as refused; real operands count in scale_fold_step_counts() only"""),
    "complex_trs4": (("traces", "operands", "energies", "refused"),
                     """complex TRS4 in a complex slab session (option complex_trs4; csrc/slab_extra.hip k_sa_trs4<double2, .>) since start: trace passes
    fused, operands Fx + sigma Gx fused, energies fused, passes refused (the vocabulary calls ran instead); slab_algebra_counts()
    counts a fused pass as the real branch does.  A pass kept out by a gate (the option off, no open complex session, several
    ranks, block form, a labelled slab form) is neither fused nor counted as refused"""),
    "column_fused": (("identity_in_place", "norms_of_differences"),
                     """operations on compressed columns done without the merge pass (csrc/column_fused.hip) since start"""),
    "block_algebra": (("operations", "fallbacks"),
                      """(operations of solver loops / C-ABI loops done on matrices in block form, fallbacks to compressed columns)"""),
}


def _define_counter(name, keys, doc, kind=dict):
    def read():
        out = (C.c_longlong * len(keys))()
        getattr(lib, "ntpoly_amd_%s_counts" % name)(out)
        values = [int(v) for v in out]
        return tuple(values) if kind is tuple else dict(zip(keys, values))
    read.__name__ = read.__qualname__ = name + "_counts"
    read.__doc__ = doc
    globals()[read.__name__] = read


for _name, _entry in _COUNTERS.items():
    _define_counter(_name, *_entry)


def last_tile_launch():
    """what the last launch of the MFMA tile kernel chose (csrc/spgemm_tile.hpp TileLaunchInfo), as a dict: `launches` since
    reset_spgemm_accum, and of the last one the instantiation `epi` (0 product, 1 X*X, 2 2X - X*X), `nw` (waves per workgroup),
    `rows` (per lane), `labelled`, `off32` (32-bit offsets), then `bsrc` (the multiplier tile: 0 prepared tiles, 1 runs through
    64-bit pointers, 2 runs through the buffer per element, 3 runs as pairs of rows), `max_kn` (largest k range of a block) and
    `skip` (1: the tile-skip test ran)"""
    out = (C.c_longlong * 9)()
    lib.ntpoly_amd_last_tile_launch(out)
    names = ("launches", "epi", "nw", "rows", "labelled", "off32", "bsrc", "max_kn", "skip")
    return {k: int(out[q]) for q, k in enumerate(names)}


def block_scope_counts():
    """(solves run in a block order across ranks, panel products of such solves on the block path)"""
    out = (C.c_longlong * 2)()
    lib.ntpoly_amd_block_scope_counts(out)
    return dict(solves=out[0], products=out[1])


def band_searches():
    """searches for a bandwidth-reducing order since start (one per sparsity pattern)"""
    out = C.c_longlong()
    lib.ntpoly_amd_band_searches(C.byref(out))
    return int(out.value)


def drop_grouped_caches():
    """forget what the grouped LDS-hash path keeps between products (the kept column orders, the table class hints, the dimensions
    whose next product goes to the grouped kernel first): the class a product starts in then does not depend on earlier products"""
    lib.ntpoly_amd_drop_grouped_caches()


@contextlib.contextmanager
def solver_session(complex_ok=True):
    """DIAGNOSTIC (like trs2_step): a session of the kind the solver loops open, held across the vocabulary calls made inside the
    `with` block -- their matrices stay in slab form between the calls, complex ones too with complex_ok (the one-call sessions
    of the C ABI do not take complex operands in slab form).  Reading a matrix back packs it, as ever."""
    lib.ntpoly_amd_session_begin(C.byref(C.c_int(1 if complex_ok else 0)))
    try:
        yield
    finally:
        lib.ntpoly_amd_session_end()


def recurrence_step(P, Tkm2, Tk, R, a, c):
    """DIAGNOSTIC, inside `with solver_session():` -- the fused recurrence step of the Chebyshev / Hermite loops on complex
    matrices (option complex_poly_sessions = 2; csrc/slab_extra.hip): Tk = P + a Tkm2 and R <- R + c Tk in one pass.
    True: taken; False: declined, every matrix as it was (the caller makes the two IncrementMatrix calls)."""
    lib.ntpoly_amd_recurrence_step.restype = C.c_int
    return bool(lib.ntpoly_amd_recurrence_step(P.ih, Tkm2.ih, Tk.ih, R.ih, d(a), d(c)))


def recurrence_step_count():
    """fused recurrence steps taken since start (option complex_poly_sessions = 2), by the Chebyshev / Hermite loops and by
    recurrence_step(); slab_algebra_counts() counts each as the two merges it replaces, a declined step counts nothing here"""
    out = C.c_longlong()
    lib.ntpoly_amd_recurrence_step_count(C.byref(out))
    return int(out.value)


def pm_session_longest_list():
    """the longest zero list an update of the fused PM loop has left on this rank since start"""
    out = C.c_longlong()
    lib.ntpoly_amd_pm_session_longest_list(C.byref(out))
    return int(out.value)


def pm_fused_step(X, Z, X2, X3, a1, a2, a3, thr, Out, Zout):
    """DIAGNOSTIC: one sigma pass and one update of the PM loop's fused path on caller-held matrices (one rank), all real or -- option
    complex_pm, FMA arithmetic -- X, X2 and X3 all complex.  Z's stored pattern is the iterate's zero list.  Returns (trace, dot) of
    X - X2 merged at thr (complex: the real parts) when taken -- Out then holds the update's non-zeros and Zout its stored zeros, in
    compressed columns of the operands' kind -- or None when refused or gated (nothing written)."""
    sc = (C.c_double * 2)()
    lib.ntpoly_amd_pm_fused_step.restype = C.c_int
    ok = lib.ntpoly_amd_pm_fused_step(X.ih, Z.ih, X2.ih, X3.ih, d(a1), d(a2), d(a3), d(thr), Out.ih, Zout.ih, sc)
    return (sc[0], sc[1]) if ok else None


def isr_chain_step(X, X2, order, a, b, c, Out1, Out2):
    """DIAGNOSTIC, inside `with solver_session():` -- one fused chain of the square-root step on caller-held matrices (X2: what the
    product X X would be).  Order 5: Out1 = (X2 + a X) + (X + b I), Out2 = (X2 + a X) + c I; order 3: Out1 = 0.375 X2 + (I - X / 2),
    Out2 untouched.  True: taken; None: refused, every matrix as it was."""
    lib.ntpoly_amd_isr_chain_step.restype = C.c_int
    ok = lib.ntpoly_amd_isr_chain_step(X.ih, X2.ih, C.byref(C.c_int(int(order))), d(a), d(b), d(c), Out1.ih, Out2.ih)
    return True if ok else None


def slab_transpose(A, AT, conjugate=False):
    """DIAGNOSTIC, one rank -- A is brought into slab form in a session of the call's own, the transpose pass runs on it (conjugate:
    the conjugate transpose) and the PACKED result is installed in AT.  True: taken; None: gated or refused, AT as it was."""
    lib.ntpoly_amd_slab_transpose.restype = C.c_int
    ok = lib.ntpoly_amd_slab_transpose(A.ih, AT.ih, C.byref(C.c_int(1 if conjugate else 0)))
    return True if ok else None


def power_vector_step(A, x, threshold):
    """DIAGNOSTIC -- one step of PowerBounds on one vector (csrc/power_vector.hip) on a caller's x: N values, complex ones for a
    complex A.  Returns (y, d1, d2, n1): y = A x, every entry the chain over ascending k in the product's arithmetic, pruned as
    the product prunes (|y_i| > threshold, else 0) and NOT scaled; d1 = sum conj(x) x, d2 = Re sum conj(x) y, n1 = sum |y|.  None:
    refused (process slices, a gather form that could not be built).  Does not depend on option power_vector; counts nothing."""
    n = A.GetActualDimension()
    kind = np.complex128 if A.IsComplex() else np.float64
    xs = np.ascontiguousarray(np.asarray(x, dtype=kind).reshape(n))
    ys = np.zeros(n, dtype=kind)
    out = (C.c_double * 3)()
    lib.ntpoly_amd_power_vector_step.restype = C.c_int
    ok = lib.ntpoly_amd_power_vector_step(A.ih, xs.ctypes.data_as(C.POINTER(C.c_double)), ys.ctypes.data_as(C.POINTER(C.c_double)),
                                          d(threshold), out)
    return (ys, float(out[0]), float(out[1]), float(out[2])) if ok else None


def cg_dots(U, V, threshold):
    """DIAGNOSTIC -- one column dot pass of CGSolver's traces (csrc/cg_dots.hip; option cg_dots: 1 for real operands, 2 for complex
    ones on one rank in FMA arithmetic) on caller-held U and V.  Returns (diag, trace): diag[j] = the real part of entry (j, j) of
    MatrixMultiply(U^H, V, threshold) for this rank's columns -- the chain over ascending k of conj(U(k, j)) V(k, j) in the product's
    arithmetic, 0.0 where the product prunes the entry or has none -- and trace = their sum in MatrixTrace's order over all ranks.
    Operands that get no slab form (not run-like) go through the same chains on compressed columns, as in the loop.  None: gated.
    Counts nothing."""
    lo, hi = U.local_columns()
    diag = np.zeros(max(0, hi - lo), dtype=np.float64)
    tr = C.c_double(0.0)
    lib.ntpoly_amd_cg_dots.restype = C.c_int
    ok = lib.ntpoly_amd_cg_dots(U.ih, V.ih, C.c_double(float(threshold)), diag.ctypes.data_as(C.POINTER(C.c_double)), C.byref(tr))
    return (diag, float(tr.value)) if ok else None


def hpcp_update_step(D1, DDH, D2DH, sigma, WH, D1out, DHout):
    """DIAGNOSTIC, inside `with solver_session():` -- one fused HPCP update on caller-held matrices, all real (option hpcp_step) or
    all complex (option complex_hpcp, one rank) (DDH, D2DH: what the products D1 (I - D1) and D1 DDH would be): D1out = (D1 + 2
    D2DH) + (-2 sigma) DDH, DHout = I - D1out, both as the vocabulary at threshold 0 builds them.  Returns the energy dot(D1out, WH)
    (complex: its real part) when taken; None: refused or gated, every matrix as it was."""
    e = C.c_double(0.0)
    lib.ntpoly_amd_hpcp_update_step.restype = C.c_int
    ok = lib.ntpoly_amd_hpcp_update_step(D1.ih, DDH.ih, D2DH.ih, d(sigma), WH.ih, D1out.ih, DHout.ih, C.byref(e))
    return float(e.value) if ok else None


def hpcp_traces_step(DDH, D2DH):
    """DIAGNOSTIC, inside `with solver_session():` -- the fused trace pass of the HPCP loop on caller-held matrices, real (option
    hpcp_step) or complex (option complex_hpcp): returns (trace(DDH), trace(D2DH)) from one pass; None: refused or gated."""
    out = (C.c_double * 2)()
    lib.ntpoly_amd_hpcp_traces_step.restype = C.c_int
    ok = lib.ntpoly_amd_hpcp_traces_step(DDH.ih, D2DH.ih, out)
    return (float(out[0]), float(out[1])) if ok else None


def scale_fold_update_step(X, X2, a, b, WH, Xout):
    """DIAGNOSTIC, inside `with solver_session():` -- one fused fold update of ScaleAndFold on caller-held matrices, all real (option
    scale_fold_step) or all complex (option complex_scale_fold, one rank) (X2: what the product X X would be): Xout = b X + a X2 as
    ScaleMatrix(X, b); IncrementMatrix(X2, X, a) at threshold 0 build it.  Returns (dot(Xout, WH), trace(Xout)) (complex: the real
    part of the dot, the sum of the real parts of the diagonal) when taken; None: refused or gated, every matrix as it was."""
    dot, tr = C.c_double(0.0), C.c_double(0.0)
    lib.ntpoly_amd_scale_fold_update_step.restype = C.c_int
    ok = lib.ntpoly_amd_scale_fold_update_step(X.ih, X2.ih, d(a), d(b), WH.ih, Xout.ih, C.byref(dot), C.byref(tr))
    return (float(dot.value), float(tr.value)) if ok else None


def scale_fold_dot_trace(X, WH):
    """DIAGNOSTIC, inside `with solver_session():` -- the pass behind the product of ScaleAndFold's scale branch, on real matrices
    (option scale_fold_step) or complex ones (option complex_scale_fold, one rank; WH as it stands: slab form, a read-only view or
    compressed columns): (dot(X, WH), trace(X)) (complex: the real part of the dot) from one pass over X and WH; None: refused or
    gated."""
    dot, tr = C.c_double(0.0), C.c_double(0.0)
    lib.ntpoly_amd_scale_fold_dot_trace.restype = C.c_int
    ok = lib.ntpoly_amd_scale_fold_dot_trace(X.ih, WH.ih, C.byref(dot), C.byref(tr))
    return (float(dot.value), float(tr.value)) if ok else None


def wom_heun_step(W, K0, K1, RK1, step, threshold, RK2out):
    """DIAGNOSTIC, inside `with solver_session():`, option wom_session = 2 -- the tail of one Heun trial of the WOM solvers on
    caller-held real matrices (csrc/wom_heun.hip): RK2out = (W + c K0) + c K1 with c = step * 0.5, as CopyMatrix and two
    IncrementMatrix calls at `threshold` build it.  Returns (err, err2) = (MatrixNorm(RK1 - RK2), MatrixNorm(RK2 - W)), each
    difference merged at `threshold`, when taken; None: refused or gated, every matrix as it was."""
    err, err2 = C.c_double(0.0), C.c_double(0.0)
    lib.ntpoly_amd_wom_heun_step.restype = C.c_int
    ok = lib.ntpoly_amd_wom_heun_step(W.ih, K0.ih, K1.ih, RK1.ih, d(step), d(threshold), RK2out.ih, C.byref(err), C.byref(err2))
    return (float(err.value), float(err2.value)) if ok else None


def wom_c_dots(X, W, XA):
    """DIAGNOSTIC, inside `with solver_session():`, option wom_session = 2 -- the two dots of WOM_C's step on caller-held real
    matrices from one kernel and one read-back: (denom, num) = (dot(X, W), dot(W, XA)); None: refused or gated."""
    out = (C.c_double * 2)()
    lib.ntpoly_amd_wom_c_dots.restype = C.c_int
    ok = lib.ntpoly_amd_wom_c_dots(X.ih, W.ih, XA.ih, out)
    return (float(out[0]), float(out[1])) if ok else None


def wom_heun_register_rows():
    """the hull of a column's four runs, in rows, up to which the Heun pass (csrc/wom_heun.hip) holds the column in registers"""
    lib.ntpoly_amd_wom_heun_register_rows.restype = C.c_int
    return int(lib.ntpoly_amd_wom_heun_register_rows())


def purify_tail_step(D, N, S, fold, Nout):
    """DIAGNOSTIC, inside `with solver_session():`, option purify_session = 2, one rank -- the tail of one iteration of PurificationExtrapolate
    on caller-held real matrices (csrc/purify_tail.hip): D the working density, N what the product D S D would be, S the overlap.
    With `fold` Nout = 2 D - N as ScaleMatrix(N, -1) and IncrementMatrix(D, N, 2) at threshold 0 build it, otherwise a copy of N.
    Returns (norm, next_trace) = (MatrixNorm(D - N'), DotMatrix(N', S)) when taken; None: refused or gated, every matrix as it was."""
    norm, nxt = C.c_double(0.0), C.c_double(0.0)
    lib.ntpoly_amd_purify_tail_step.restype = C.c_int
    ok = lib.ntpoly_amd_purify_tail_step(D.ih, N.ih, S.ih, C.byref(C.c_int(1 if fold else 0)), Nout.ih, C.byref(norm), C.byref(nxt))
    return (float(norm.value), float(nxt.value)) if ok else None


def pade_chain_step(Base, addends, scales, coeffs, Out1, Out2):
    """DIAGNOSTIC, inside `with solver_session():`, option pade_session = 2, one rank -- one of the two groups of merges of
    ComputeExponentialPade on caller-held real matrices (csrc/pade_chain.hip): for q = 1, 2
    Out_q = CopyMatrix(Base); ScaleMatrix(Out_q, scales[q - 1]); IncrementMatrix(addends[k], Out_q, coeffs[q - 1][k], threshold 0)
    for every k.  `addends`: 1 or 3 matrices; `coeffs`: two rows of len(addends) numbers.  Returns True when taken (both outputs
    packed); None: refused or gated, every matrix as it was."""
    addends = list(addends)
    m = len(addends)
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).reshape(-1))
    s = np.ascontiguousarray(np.asarray(scales, dtype=np.float64).reshape(-1))
    if m == 0 or c.size != 2 * m or s.size != 2:
        raise ValueError("pade_chain_step: two scales and two rows of len(addends) coefficients")
    ih = [a.ih for a in addends[:3]] + [addends[0].ih] * max(0, 3 - m)
    lib.ntpoly_amd_pade_chain_step.restype = C.c_int
    ok = lib.ntpoly_amd_pade_chain_step(Base.ih, ih[0], ih[1], ih[2], C.byref(C.c_int(m)), s.ctypes.data_as(C.POINTER(C.c_double)),
                                        c.ctypes.data_as(C.POINTER(C.c_double)), Out1.ih, Out2.ih)
    return True if ok else None


def poly_step(P, Tkm2, R, a, c, TkOut, ROut):
    """DIAGNOSTIC, inside `with solver_session():`, option poly_step = 2, one rank -- the tail of a step of the real Chebyshev /
    Hermite recurrences on caller-held real matrices (csrc/poly_step.hip): TkOut = what IncrementMatrix(Tkm2, P, a, threshold 0)
    leaves in P, ROut = what IncrementMatrix(TkOut, R, c, threshold 0) then leaves in R, both from one pass and packed.  TkOut and
    ROut are none of the inputs and not one another; the inputs keep their values.  Returns True when taken; False: refused or
    gated, every matrix as it was."""
    lib.ntpoly_amd_poly_step.restype = C.c_int
    ok = lib.ntpoly_amd_poly_step(P.ih, Tkm2.ih, R.ih, C.byref(C.c_double(float(a))), C.byref(C.c_double(float(c))), TkOut.ih, ROut.ih)
    return bool(ok)


def sum_chain(Base, s, addends, coeffs, post, Out):
    """DIAGNOSTIC, inside `with solver_session():`, option sum_chain = 1, one rank -- the scaled sum chain of the real solver loops
    on caller-held real matrices (csrc/sum_chain.hip): Out = CopyMatrix(Base); ScaleMatrix(Out, s); IncrementMatrix(addends[k], Out,
    coeffs[k], threshold 0) for every k; ScaleMatrix(Out, post), from one pass and packed (s = 1 and post = 1 stand for no scaling
    call).  `addends`: 1 to 5 matrices; `coeffs`: as many numbers.  Out is Base or none of the inputs; the inputs keep their values.
    Returns True when taken; False: refused or gated, every matrix as it was.  Operands that are ALL complex take the same chain on
    (re, im) pairs with option complex_sum_chain = 2 inside `with solver_session(True):` (counted in complex_sum_chain_counts()
    only); real and complex operands mixed are a gate."""
    addends = list(addends)
    m = len(addends)
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).reshape(-1))
    if c.size != m:
        raise ValueError("sum_chain: one coefficient per addend")
    ih = (C.POINTER(C.c_int) * max(m, 1))(*[C.cast(a.ih, C.POINTER(C.c_int)) for a in addends])
    lib.ntpoly_amd_sum_chain.restype = C.c_int
    ok = lib.ntpoly_amd_sum_chain(Base.ih, C.byref(C.c_double(float(s))), C.byref(C.c_int(m)), ih, c.ctypes.data_as(C.POINTER(C.c_double)),
                                  C.byref(C.c_double(float(post))), Out.ih)
    return bool(ok)


def trs4_chain_step(X, X2, sigma, P):
    """DIAGNOSTIC, inside `with solver_session():` -- TRS4's chain on caller-held matrices, real or (option complex_trs4) complex
    (X2: what the product X X would be): P = (4 X - 3 X2) + sigma (I - 2 X + X2) as the vocabulary at threshold 0 builds it.
    Returns (dot(X2, 4 X - 3 X2), dot(X2, I - 2 X + X2)), the real parts, when taken; None: refused or gated (sigma == 0), every
    matrix as it was."""
    tf, tg = C.c_double(0.0), C.c_double(0.0)
    lib.ntpoly_amd_trs4_chain_step.restype = C.c_int
    ok = lib.ntpoly_amd_trs4_chain_step(X.ih, X2.ih, d(sigma), P.ih, C.byref(tf), C.byref(tg))
    return (float(tf.value), float(tg.value)) if ok else None


def trs4_energy(X, WH):
    """DIAGNOSTIC, inside `with solver_session():` -- the energy pass of the complex TRS4 loop (option complex_trs4): the real part
    of dot(X, WH) from one pass over the runs of a complex X and WH as it stands (slab form or compressed columns, stored zeros
    included); None: refused or gated."""
    e = C.c_double(0.0)
    lib.ntpoly_amd_trs4_energy.restype = C.c_int
    ok = lib.ntpoly_amd_trs4_energy(X.ih, WH.ih, C.byref(e))
    return float(e.value) if ok else None


def last_grouped_stats():
    """grouped LDS-hash path of the last SpGEMM (csrc/spgemm_grouped.hip)"""
    out = (C.c_longlong * 6)()
    r = C.c_double()
    lib.ntpoly_amd_last_grouped_stats(out, C.byref(r))
    return dict(used=int(out[0]), failed_cols=int(out[1]), groups=int(out[2]), level=int(out[3]), minhash=int(out[4]),
                tile_rows=int(out[5]), union_ratio=r.value)


def last_block_stats():
    """block path of the last SpGEMM (csrc/spgemm_block.hip: 16 x 16 tiles of a clustered index order on the FP64 matrix cores)"""
    out = (C.c_longlong * 3)()
    r = C.c_double()
    lib.ntpoly_amd_last_block_stats(out, C.byref(r))
    return dict(used=int(out[0]), tile_products=int(out[1]), candidates=int(out[2]), fill=r.value)


def last_spgemm_thin():
    """1: the last SpGEMM ran on the thin-left kernel (csrc/spgemm_thin.hip)"""
    lib.ntpoly_amd_last_spgemm_thin.restype = C.c_int
    return int(lib.ntpoly_amd_last_spgemm_thin())


def block_order(M):
    """position of every index in the block order the engine multiplies matrices of M's dimension in (made from M if none exists)"""
    pos = np.zeros(M.GetActualDimension(), dtype=np.int32)
    lib.ntpoly_amd_block_order.restype = C.c_int
    ok = lib.ntpoly_amd_block_order(M.ih, pos.ctypes.data_as(C.c_void_p))
    return pos if ok else None


def block_order_of_pattern(M):
    """(positions, super-blocks) of the block order made FOR M's pattern (what a solve in a block order across ranks redistributes
    its operands in; complex M: made from the moduli), or None where there is none"""
    pos = np.zeros(M.GetActualDimension(), dtype=np.int32)
    ns = C.c_int()
    lib.ntpoly_amd_block_order_of_pattern.restype = C.c_int
    ok = lib.ntpoly_amd_block_order_of_pattern(M.ih, pos.ctypes.data_as(C.c_void_p), C.byref(ns))
    return (pos, int(ns.value)) if ok else None


def increment_identity(Identity, B, alpha):
    """IncrementMatrix(Identity, B, alpha) as the solver loops call it (in place where every column stores its diagonal)"""
    lib.ntpoly_amd_increment_identity(Identity.ih, B.ih, d(alpha))


def norm_axpby(A, B, alpha, beta):
    """MatrixNorm(alpha A + beta B) without forming it; None when the engine would form the difference"""
    r = C.c_double()
    lib.ntpoly_amd_norm_axpby.restype = C.c_int
    ok = lib.ntpoly_amd_norm_axpby(A.ih, B.ih, d(alpha), d(beta), C.byref(r))
    return r.value if ok else None


def drop_block_caches():
    lib.ntpoly_amd_drop_block_caches()


def exchange_stats():
    """(halo exchanges of distributed multiplies so far, host synchronisations inside them, ALL host synchronisations of
    the process so far) -- the synchronisations are counted where the host waits (sync_stream in csrc/common.cpp)"""
    out = (C.c_longlong * 3)()
    lib.ntpoly_amd_exchange_stats(out)
    return int(out[0]), int(out[1]), int(out[2])


def reset_spgemm_accum():
    lib.ntpoly_amd_reset_spgemm_accum()


def spgemm_accum():
    out = (C.c_longlong * 3)()
    dd = (C.c_double * 3)()
    lib.ntpoly_amd_get_spgemm_accum(out, dd)
    return dict(calls=out[0], products=out[1], nnz_c=out[2], alg_bytes=dd[0], ms_numeric=dd[1], ms_total=dd[2])


def solver_trace():
    n = int(lib.ntpoly_amd_trace_iterations())
    v = np.zeros(n)
    e = np.zeros(n)
    sg = np.zeros(n)
    nz = np.zeros(n, dtype=np.int64)
    if n:
        lib.ntpoly_amd_trace_get(v.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                 sg.ctypes.data_as(C.c_void_p), nz.ctypes.data_as(C.c_void_p))
    a, c = C.c_double(), C.c_double()
    lib.ntpoly_amd_trace_times(C.byref(a), C.byref(c))
    return dict(iterations=n, value=v, energy=e, sigma=sg, nnz=nz, setup_ms=a.value, loop_ms=c.value)


def malloc_stats():
    n, ms = C.c_longlong(), C.c_double()
    lib.ntpoly_amd_malloc_stats(C.byref(n), C.byref(ms))
    return n.value, ms.value


def release_cache():
    """frees what the engine keeps on the device between solves (operand caches, kept transposes) -- ntpoly_amd_release_cache"""
    lib.ntpoly_amd_release_cache()


def memory():
    a, c = C.c_longlong(), C.c_longlong()
    lib.ntpoly_amd_memory(C.byref(a), C.byref(c))
    return a.value, c.value
