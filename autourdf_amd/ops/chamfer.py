"""K1 / K3: L1 nearest neighbour both ways, the Chamfer loss and the cluster transform, with their autograd glue."""
import torch

from .. import _lib
from ._common import _need, _p, _stream, _workspace


def nn_l1_bidir(x: torch.Tensor, y: torch.Tensor):
    """x (nx,3), y (ny,3) fp32 -> (dx, ix, dy, iy): L1 nearest neighbour both ways, first min wins."""
    L = _lib.load()
    x, y = _need(x, torch.float32, "x"), _need(y, torch.float32, "y")
    nx, ny = x.shape[0], y.shape[0]
    if nx == 0 or ny == 0:
        raise ValueError("nn_l1_bidir: empty point cloud")      # pytorch3d rejects it as well
    dx = torch.empty(nx, dtype=torch.float32, device=x.device)
    dy = torch.empty(ny, dtype=torch.float32, device=x.device)
    ix = torch.empty(nx, dtype=torch.int64, device=x.device)
    iy = torch.empty(ny, dtype=torch.int64, device=x.device)
    _lib.check(L.creg_nn_l1_bidir_f32(_p(x), nx, _p(y), ny, _p(dx), _p(ix), _p(dy), _p(iy), _stream()),
               "creg_nn_l1_bidir_f32")
    return dx, ix, dy, iy


class _ChamferL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        L = _lib.load()
        dx, ix, dy, iy = nn_l1_bidir(x, y)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        _lib.check(L.creg_chamfer_l1_reduce_f32(_p(dx), dx.numel(), _p(dy), dy.numel(), _p(loss), _stream()),
                   "creg_chamfer_l1_reduce_f32")
        ctx.save_for_backward(x.detach().contiguous(), y.detach().contiguous(), ix, iy)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        x, y, ix, iy = ctx.saved_tensors
        nx, ny = x.shape[0], y.shape[0]
        grad = torch.empty_like(x)
        scratch = _workspace(x.device, L.creg_nn_l1_bwd_scratch_bytes(nx))
        one = torch.tensor(1.0, dtype=torch.float32)
        gx, gy = float(one / nx), float(one / ny)
        _lib.check(L.creg_nn_l1_bwd_f32(_p(x), nx, _p(y), ny, _p(ix), _p(iy), gx, gy, _p(grad), _p(scratch),
                                        _stream()), "creg_nn_l1_bwd_f32")
        return grad * g, None


def chamfer_distance(x: torch.Tensor, y: torch.Tensor, norm: int = 1):
    """pytorch3d.loss.chamfer_distance(x, y, norm=1) for the reference's call (mlp_reg.py:96):
    x (1,P1,3) with grad, y (1,P2,3); returns (loss, None)."""
    if norm != 1:
        raise NotImplementedError("only norm=1 is on the registration path")
    if x.dim() != 3 or x.shape[0] != 1 or y.shape[0] != 1:
        raise NotImplementedError("batch of 1 only (as the reference calls it)")
    return _ChamferL1.apply(_need(x[0], torch.float32, "x"), _need(y[0], torch.float32, "y")), None


class _ClusterTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, offsets, M):
        L = _lib.load()
        out = torch.empty_like(pts)
        k = M.shape[0]
        _lib.check(L.creg_cluster_transform_f32(_p(pts), pts.shape[0], _p(offsets), k, _p(M), _p(out), _stream()),
                   "creg_cluster_transform_f32")
        ctx.save_for_backward(pts, offsets)
        ctx.k = k
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.load()
        pts, offsets = ctx.saved_tensors
        gM = torch.empty(ctx.k, 4, 4, dtype=torch.float32, device=pts.device)
        _lib.check(L.creg_cluster_transform_bwd_f32(_p(pts), _p(offsets), ctx.k, _p(g.contiguous()), _p(gM), _stream()),
                   "creg_cluster_transform_bwd_f32")
        return None, None, gM


def cluster_transform(pts: torch.Tensor, offsets: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """pts (n,3) fp32 clusters back to back, offsets (k+1) int32, M (k,4,4) fp32 -> world points."""
    return _ClusterTransform.apply(_need(pts, torch.float32, "pts"), _need(offsets, torch.int32, "offsets"),
                                   _need(M, torch.float32, "M"))


def pack_clusters(clusters, device, dtype=torch.float32):
    """list of (M_k,3) tensors/arrays -> (flat (n,3) tensor, offsets (k+1) int32 tensor), on `device`."""
    ts = [torch.as_tensor(c, dtype=dtype).reshape(-1, 3) for c in clusters]
    sizes = [t.shape[0] for t in ts]
    off = torch.zeros(len(ts) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0).to(torch.int32)
    flat = torch.cat([t.to(device) for t in ts], 0) if ts else torch.zeros(0, 3, dtype=dtype, device=device)
    return flat.contiguous(), off.to(device)
