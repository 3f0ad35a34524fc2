"""K5: the row-wise pose conversions (SE(3), dual quaternions, quaternions, rotation matrices)."""
import torch

from .. import _lib
from ._common import _need, _p, _stream


def _rows(fn_name, a, out_shape, b=None, out2_shape=None):
    L = _lib.load()
    a = _need(a, torch.float32, "input")
    k = a.shape[0]
    out = torch.empty((k,) + out_shape, dtype=torch.float32, device=a.device)
    fn = getattr(L, fn_name)
    if k == 0:                                   # an empty tensor's data pointer is null, which the C ABI rejects
        return (out, torch.empty((0,) + out2_shape, dtype=torch.float32, device=a.device)) if out2_shape is not None else out
    if out2_shape is not None:
        out2 = torch.empty((k,) + out2_shape, dtype=torch.float32, device=a.device)
        _lib.check(fn(_p(a), k, _p(out), _p(out2), _stream()), fn_name)
        return out, out2
    if b is not None:
        b = _need(b, torch.float32, "input")
        _lib.check(fn(_p(a), _p(b), k, _p(out), _stream()), fn_name)
    else:
        _lib.check(fn(_p(a), k, _p(out), _stream()), fn_name)
    return out


def se3_to_dq(M): return _rows("creg_se3_to_dq_f32", M, (8,))
def dq_to_se3(dq): return _rows("creg_dq_to_se3_f32", dq, (4, 4))
def dq_to_se3_bwd(dq, gM): return _rows("creg_dq_to_se3_bwd_f32", dq, (8,), b=gM)
def dq_multiply(a, b): return _rows("creg_dq_multiply_f32", a, (8,), b=b)
def dq_invert(dq): return _rows("creg_dq_invert_f32", dq, (8,))
def dq_to_quat_trans(dq): return _rows("creg_dq_to_quat_trans_f32", dq, (4,), out2_shape=(3,))
def quat_trans_to_dq(q, t): return _rows("creg_quat_trans_to_dq_f32", q, (8,), b=t)
def matrix_to_quat(R): return _rows("creg_matrix_to_quat_f32", R, (4,))
def quat_to_matrix(q): return _rows("creg_quat_to_matrix_f32", q, (3, 3))
