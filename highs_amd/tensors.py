"""Problems, updates and solutions as torch tensors that are in HBM already (pdlp_mi355x_create_device, _update_device,
_run_device: include/pdlp_mi355x.h, "device-resident entries").

TensorProblem has the fields of lp.HighsLp, Hessian included, as tensors: int32 starts and indices, float64 values,
contiguous, all on ONE cuda device.  Dtype, contiguity and device are checked here, in Python (TypeError / ValueError);
whether a pointer really is device memory is checked once more by the library before it launches anything.

torch is imported inside the functions that need it: `import highs_amd` works without it.
"""
import ctypes as C

from . import abi

def init():
    """Load the library and torch and check that they share ONE copy of the HIP runtime -> its path.  A PyTorch wheel
    bundles a libamdhip64 of its own; tensors and solver must live in the same copy (the second one to start finds no
    device).  solver.lib() arranges that for either import order (see there); this raises where it did not work — the
    library's runtime was brought in by other means before torch.  Called by TensorProblem.from_lp and from_tensors."""
    import os

    from . import solver

    solver.lib()
    import torch  # noqa: F401

    try:
        with open("/proc/self/maps") as f:
            copies = sorted({os.path.realpath(line.split()[-1]) for line in f if "libamdhip64" in line})
    except OSError:
        return None
    if len(copies) > 1:
        raise RuntimeError("two copies of the HIP runtime are loaded (%s): tensors made by one are no device memory to the "
                           "other.  Import torch, or call highs_amd.solver.lib(), before anything else loads libamdhip64"
                           % ", ".join(copies))
    return copies[0] if copies else None


def check_tensor(name, t, dtype_name, count=None, device=None):
    """t is a contiguous tensor of the dtype on a cuda device (`device`, where given) with `count` elements (where given).
    TypeError for what is no tensor or has the wrong dtype; ValueError for layout, device and size."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor is needed, got {type(t).__name__}")
    want = getattr(torch, dtype_name)
    if t.dtype != want:
        raise TypeError(f"{name}: dtype {want} is needed, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{name}: a one-dimensional tensor is needed, got {t.dim()} dimensions")
    if not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous tensor is needed")
    if t.device.type != "cuda":
        raise ValueError(f"{name}: a tensor on a cuda device is needed, got one on {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: is on {t.device}, the other arrays are on {device}")
    if count is not None and t.numel() != count:
        raise ValueError(f"{name}: {count} elements are needed, got {t.numel()}")
    return t


def device_ordinal(device):
    """The HIP ordinal of a torch cuda device (the current one where the device carries no index)."""
    import torch

    return device.index if device.index is not None else torch.cuda.current_device()


def pointer(t, ctype):
    """The address of a tensor's first element as a ctypes pointer (NULL for None)."""
    return None if t is None else C.cast(C.c_void_p(t.data_ptr()), ctype)


class TensorProblem:
    """lp.HighsLp with every array a tensor on one cuda device.  hessian: (q_start, q_index, q_value) or None."""

    def __init__(self, num_col, num_row, col_cost, col_lower, col_upper, row_lower, row_upper, a_start, a_index, a_value,
                 sense=1, offset=0.0, hessian=None):
        self.num_col, self.num_row = int(num_col), int(num_row)
        self.sense, self.offset = int(sense), float(offset)
        self.a_start = check_tensor("a_start", a_start, "int32", self.num_col + 1)
        dev = self.a_start.device
        self.device = dev
        self.col_cost = check_tensor("col_cost", col_cost, "float64", self.num_col, dev)
        self.col_lower = check_tensor("col_lower", col_lower, "float64", self.num_col, dev)
        self.col_upper = check_tensor("col_upper", col_upper, "float64", self.num_col, dev)
        self.row_lower = check_tensor("row_lower", row_lower, "float64", self.num_row, dev)
        self.row_upper = check_tensor("row_upper", row_upper, "float64", self.num_row, dev)
        self.a_index = check_tensor("a_index", a_index, "int32", None, dev)
        self.a_value = check_tensor("a_value", a_value, "float64", self.a_index.numel(), dev)
        self.num_nz = int(self.a_index.numel())
        self.hessian = None
        if hessian is not None:
            qs = check_tensor("q_start", hessian[0], "int32", None, dev)
            qi = check_tensor("q_index", hessian[1], "int32", None, dev)
            qv = check_tensor("q_value", hessian[2], "float64", qi.numel(), dev)
            if qs.numel() < 1 or qs.numel() - 1 > self.num_col:
                raise ValueError(f"q_start: between 1 and num_col + 1 = {self.num_col + 1} elements are needed, got {qs.numel()}")
            self.hessian = (qs, qi, qv)

    @classmethod
    def from_lp(cls, lp, device="cuda"):
        """Upload a HighsLp (numpy arrays) once; afterwards the problem lives on `device`."""
        import numpy as np
        import torch

        init()
        dev = torch.device(device)
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy()).to(dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).copy()).to(dev)
        hess = getattr(lp, "hessian", None)
        return cls(lp.num_col, lp.num_row, f64(lp.col_cost), f64(lp.col_lower), f64(lp.col_upper), f64(lp.row_lower),
                   f64(lp.row_upper), i32(lp.a_start), i32(lp.a_index), f64(lp.a_value), lp.sense, lp.offset,
                   None if hess is None else (i32(hess[0]), i32(hess[1]), f64(hess[2])))

    def struct(self, start=None):
        """-> (abi.PdlpProblem whose array pointers are the tensors' addresses, the tensors it needs kept alive).
        start: dict with col_value, row_value, row_dual as tensors (all three), or None."""
        P = abi.PdlpProblem()
        P.num_col, P.num_row, P.num_nz = self.num_col, self.num_row, self.num_nz
        P.a_start = pointer(self.a_start, abi.c_i32p)
        P.a_index = pointer(self.a_index, abi.c_i32p)
        P.a_value = pointer(self.a_value, abi.c_f64p)
        for name in ("col_cost", "col_lower", "col_upper", "row_lower", "row_upper"):
            setattr(P, name, pointer(getattr(self, name), abi.c_f64p))
        P.offset, P.sense = self.offset, self.sense
        keep = [self]
        if start is not None:
            sc = check_tensor("start col_value", start["col_value"], "float64", self.num_col, self.device)
            sv = check_tensor("start row_value", start["row_value"], "float64", self.num_row, self.device)
            sd = check_tensor("start row_dual", start["row_dual"], "float64", self.num_row, self.device)
            P.start_col_value, P.start_row_value, P.start_row_dual = (pointer(t, abi.c_f64p) for t in (sc, sv, sd))
            P.start_value_valid = P.start_dual_valid = 1
            keep += [sc, sv, sd]
        if self.hessian is not None:
            qs, qi, qv = self.hessian
            P.q_dim = qs.numel() - 1
            P.q_start, P.q_index, P.q_value = pointer(qs, abi.c_i32p), pointer(qi, abi.c_i32p), pointer(qv, abi.c_f64p)
        return P, keep


class TensorUpdate:
    """A pdlp_update_t whose arrays are tensors (None = unchanged), checked against the solver's sizes and device."""

    def __init__(self, num_col, num_row, device, col_cost=None, col_lower=None, col_upper=None, row_lower=None, row_upper=None,
                 offset=None, start=None):
        U = abi.PdlpUpdate()
        self.keep = []

        def put(field, label, t, count):
            if t is None:
                return
            check_tensor(label, t, "float64", count, device)
            self.keep.append(t)
            setattr(U, field, pointer(t, abi.c_f64p))

        put("col_cost", "col_cost", col_cost, num_col)
        put("col_lower", "col_lower", col_lower, num_col)
        put("col_upper", "col_upper", col_upper, num_col)
        put("row_lower", "row_lower", row_lower, num_row)
        put("row_upper", "row_upper", row_upper, num_row)
        if offset is not None:
            U.offset, U.has_offset = float(offset), 1
        if start is not None:  # (partial input is passed on as it is: the library refuses it with its own message)
            put("start_col_value", "start col_value", start.get("col_value"), num_col)
            put("start_row_value", "start row_value", start.get("row_value"), num_row)
            put("start_row_dual", "start row_dual", start.get("row_dual"), num_row)
        self.struct = U


class TensorVariant:
    """A pdlp_variant_t whose arrays are tensors: one variant of DeviceBatch.run_tensors — a_value / q_value (None = the
    values of the batch's problem), iter_limit for this variant alone, and the arguments of TensorUpdate.  Rows of a
    contiguous [K, n] tensor are valid arrays."""

    def __init__(self, num_col, num_row, device, a_value=None, q_value=None, iter_limit=None, **update):
        self.update = TensorUpdate(num_col, num_row, device, **update)
        V = abi.PdlpVariant()
        self.keep = list(self.update.keep)
        if a_value is not None:
            check_tensor("a_value", a_value, "float64", None, device)
            V.a_value, V.num_nz = pointer(a_value, abi.c_f64p), a_value.numel()
            self.keep.append(a_value)
        if q_value is not None:
            check_tensor("q_value", q_value, "float64", None, device)
            V.q_value, V.num_q_nz = pointer(q_value, abi.c_f64p), q_value.numel()
            self.keep.append(q_value)
        V.u = self.update.struct
        if iter_limit is not None:
            V.u.reserved = int(iter_limit)
        self.struct = V


def stacked(**two_d):
    """Stacked tensors -> the list of variants DeviceBatch.run_tensors takes: stacked(col_cost=C, a_value=A) with C of
    shape [K, num_col] and A of shape [K, num_nz] is [dict(col_cost=C[0], a_value=A[0]), ..., dict(col_cost=C[K-1], ...)].
    Every tensor is two-dimensional with the same first dimension (ValueError otherwise); None entries are left out."""
    import torch

    K = None
    for name, t in two_d.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a torch tensor is needed, got {type(t).__name__}")
        if t.dim() != 2:
            raise ValueError(f"{name}: a two-dimensional tensor [K, n] is needed, got {t.dim()} dimensions")
        if K is not None and t.shape[0] != K:
            raise ValueError(f"{name}: {K} rows are needed as in the other arrays, got {t.shape[0]}")
        K = t.shape[0]
    if K is None:
        raise ValueError("stacked: no tensor given")
    return [{name: t[k] for name, t in two_d.items() if t is not None} for k in range(K)]


class TensorResult:
    """What run_tensors returns: the four vectors as tensors on the solver's device and the scalars of pdlp_result_t
    (attribute access falls through to the struct: term_code, num_iter, primal_obj, setup_seconds, ...).  A vector named
    in `skip` is not asked for: its pointer is NULL and its tensor None."""

    VECTORS = ("col_value", "col_dual", "row_value", "row_dual")

    def __init__(self, num_col, num_row, device, out=None, skip=()):
        import torch

        sizes = dict(col_value=num_col, col_dual=num_col, row_value=num_row, row_dual=num_row)
        out = dict(out or {})
        unknown = (set(out) | set(skip)) - set(self.VECTORS)
        if unknown:
            raise ValueError(f"out: unknown vectors {sorted(unknown)}; the four are {self.VECTORS}")
        R = abi.PdlpResult()
        self.tensors = {}
        for name in self.VECTORS:
            t = out.get(name)
            if name in skip:
                self.tensors[name] = None
                continue
            if t is None:
                t = torch.empty(sizes[name], dtype=torch.float64, device=device)
            else:
                check_tensor("out[%r]" % name, t, "float64", sizes[name], device)
            self.tensors[name] = t
            setattr(R, name, pointer(t, abi.c_f64p))
        self.struct = R

    def __getattr__(self, k):
        d = self.__dict__
        if k in d.get("tensors", {}):
            return d["tensors"][k]
        return getattr(d["struct"], k)
