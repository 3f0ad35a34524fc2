"""What every stage's wrappers share: the stream, the tensor check, pointers, workspaces, offset checks, the joint table."""
import ctypes

import numpy as np

import torch


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor on the MI355X (autourdf_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _workspace(dev, nbytes):
    """The workspace a ``*_workspace_bytes`` / ``*_scratch_bytes`` call asks for: ``max(nbytes, 1)`` bytes as uint8 on ``dev`` (the
    allocator's alignment is far above the 8 the entries need).  The caller passes ``_p(ws)`` and the library's own ``nbytes``;
    a size of 0 ("unsupported sizes") is the entry's to refuse."""
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)


def _ptr_array(tensors):
    """The ``void*[B]`` of a batch entry's per-problem arrays."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _host_offsets_ok(off, n):
    """Do the numpy offsets ``off`` (at least one entry) run from 0 to n without decreasing?"""
    return off[0] == 0 and off[-1] == n and not np.any(np.diff(off) < 0)


def _device_offsets_ok(off, n):
    """``_host_offsets_ok`` for a device tensor -> a 0-d bool tensor.  Nothing is read back here: the caller folds it into its other
    conditions and synchronises once."""
    return (off[0] == 0) & (off[-1] == n) & (off[1:] >= off[:-1]).all()


def _shapes_expected(who, arrays):
    """The ValueError that names every array with the expected and the received shape."""
    return ValueError(f"{who}: {' / '.join(f'{name} {want}' for name, want, _ in arrays)} expected, got "
                      f"{', '.join(str(tuple(t.shape)) for _, _, t in arrays)}")


def joint_chains(table):
    """chain (L) uint64 of a joint table (``UrdfRobot.fk_table()``): bit j of chain[l] is set iff joint j lies on the path from the
    root to link l.  The table is in topological order, so a child's mask is its parent's plus its own bit; a joint with an index
    outside [0, L) sets no bit, as the forward kinematics skips it.  At most 64 joints."""
    n_links, parent, child = int(table["n_links"]), np.asarray(table["parent"]), np.asarray(table["child"])
    if len(parent) > 64:
        raise ValueError(f"joint_chains: at most 64 joints fit a mask, got {len(parent)}")
    chain = [0] * n_links
    for j, (pa, ch) in enumerate(zip(parent, child)):
        if 0 <= pa < n_links and 0 <= ch < n_links:
            chain[ch] = chain[pa] | (1 << j)
    return np.array(chain, np.uint64)


def _table_on(dev, table, chains=False):
    """A joint table's arrays on ``dev``: (parent, child, type, origin, axis), then the ``joint_chains`` masks as int64 when
    ``chains``.  They go up once per robot and device and are kept in the dict, under ``_dev`` and ``_dev_fit`` (with the masks);
    nothing else reads or writes those keys.  To change a table, change a copy without them:
    ``{k: v for k, v in table.items() if not k.startswith("_dev")}``."""
    key = "_dev_fit" if chains else "_dev"
    tdev = table.get(key)
    if tdev is None or tdev[0].device != dev:
        tdev = tuple(torch.as_tensor(np.ascontiguousarray(table[k]), device=dev) for k in ("parent", "child", "type", "origin", "axis"))
        if chains:
            tdev += (torch.as_tensor(joint_chains(table).view(np.int64), device=dev),)
        table[key] = tdev
    return tdev
