"""A1: the device-resident train plan."""
import ctypes

import numpy as np

import torch

from .. import _lib
from ._common import _need, _p, _stream

Q_PARAM_ORDER = ["encoder.0.weight", "encoder.0.bias", "decoder_1.0.weight", "decoder_1.0.bias",
                 "decoder_1.2.weight", "decoder_1.2.bias", "decoder_2.0.weight", "decoder_2.0.bias",
                 "decoder_2.2.weight", "decoder_2.2.bias"]
DQ_PARAM_ORDER = ["encoder.0.weight", "encoder.0.bias", "decoder.0.weight", "decoder.0.bias",
                  "decoder.2.weight", "decoder.2.bias"]
#: creg_train_shape.rot: the reference's four --r choices (mlp_reg.py:64-90).  RRegMLP ('6d') and RegMLP ('rpy') name their
#: tensors like QRegMLP (model_utils.py:170-281): Q_PARAM_ORDER serves the three.
TRAIN_ROT = {"q": 0, "dq": 1, "6d": 2, "rpy": 3}
#: per rot: (input features of the encoder = 8 x the pose row's width, outputs of decoder_2)
_TWO_DECODER = {0: (56, 4), 2: (72, 6), 3: (48, 3)}


TRAIN_HIDDEN_TILES = (64, 128, 256, 512)      # widths the train kernels are instantiated for


class TrainPlan:
    """Device-resident `train` loop (mlp_reg.py:17-152) for one (rot, K, hidden, N) shape.

    `hidden` may be any width up to 512, like the reference's models (model_utils.py:65-168): a width the kernels are not
    instantiated for runs on the next one that is, with the extra units' weights and biases zero.  Such a unit's activation is
    exactly 0 (LeakyReLU / ReLU of 0), it adds exactly 0 to every sum it enters, and every gradient of its parameters is a
    product with that 0 or with the zero column that leads out of it -- so Adam leaves them at 0 and the trained model, losses
    and poses are those of the unpadded model; the caller's tensors keep their own shapes.

    `rot`: 'q' / 'dq' / '6d' / 'rpy' -- the reference's four --r choices (mlp_reg.py:64-90); `params` in Q_PARAM_ORDER (DQ_PARAM_ORDER
    for 'dq').  `graph_branches`: creg_train_shape.graph_branches (include/creg.h) -- 0 = chain streams, the library's count."""

    def __init__(self, rot: str, k: int, hidden: int, n_pred: int, n_tgt: int, epochs: int = 300,
                 use_graph: bool = True, device=None, batch: int = 1, graph_branches: int = 0,
                 nn_search: int = 0):
        self.L = _lib.load()
        self.rot = TRAIN_ROT[rot]
        self.device = _lib.device(torch.device(device) if device is not None else None)
        self.batch = int(batch)
        self.hidden_model = int(hidden)                                     # the caller's width
        if hidden < 2 or hidden > TRAIN_HIDDEN_TILES[-1]:
            raise ValueError(f"unsupported train shape: hidden {hidden} (2 .. {TRAIN_HIDDEN_TILES[-1]})")
        hidden = next(t for t in TRAIN_HIDDEN_TILES if t >= hidden)         # the width the kernels run at
        self.shape = _lib.TrainShape(self.rot, k, hidden, epochs, n_pred, n_tgt, int(use_graph), self.batch,
                                     int(graph_branches), int(nn_search))
        need = self.L.creg_train_workspace_bytes(ctypes.byref(self.shape))
        if need == 0:
            raise ValueError(f"unsupported train shape (rot {rot!r}, k = {k}, hidden {hidden}): the plan takes 1 <= k <= 256 clusters (fewer for --r 6d at hidden 512: the backward's LDS tiles) "
                             "and hidden widths up to 512 (include/creg.h, creg_train_shape)")
        self.ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)      # the plan wants 256-byte alignment: room to round the base up
        base = (self.ws.data_ptr() + 255) // 256 * 256
        self.plan = ctypes.c_void_p()
        _lib.check(self.L.creg_train_plan_create(ctypes.byref(self.shape), ctypes.c_void_p(base), need,
                                                 ctypes.byref(self.plan)), "creg_train_plan_create")
        self.k, self.n_pred, self.n_tgt, self.epochs, self.hidden = k, n_pred, n_tgt, epochs, hidden
        info = (ctypes.c_int32 * 9)()
        _lib.check(self.L.creg_train_plan_info(self.plan, info), "creg_train_plan_info")
        #: what the plan chose from its shape (never a result): searches, graph branches, problems per launch, epochs per graph
        self.info = {"pruned_target_search": bool(info[0]), "pruned_predicted_search": bool(info[1]), "graph_branches": int(info[2]),
                     "batch": int(info[3]), "epochs_per_graph": int(info[4]), "nn_points_per_lane": int(info[5]),
                     "nn_boxes_per_lane": (int(info[6]), int(info[7])), "nn_queries_per_wave": 16 if int(info[0]) == 2 else 4}
        if nn_search == 0 and not (self.info["pruned_target_search"] and self.info["pruned_predicted_search"]):
            import warnings
            which = [d for d, on in (("predicted -> target", self.info["pruned_target_search"]),
                                     ("target -> predicted", self.info["pruned_predicted_search"])) if not on]
            warnings.warn(f"creg train plan (k={k}, n_pred={n_pred}, n_tgt={n_tgt}): exhaustive nearest-neighbour search in the "
                          f"{' and '.join(which)} direction(s) -- the shape is beyond the block-pruned search's limits "
                          "(n_tgt <= 65536: four chunks of k-d leaves built in LDS; n_pred < 65535 and at most 512 blocks of the padded "
                          "predicted cloud); same results, several times the launch time", RuntimeWarning, stacklevel=2)

    def chain_probe_us(self) -> int:
        """creg_train_plan_info_t.chain_probe_us AFTER a run: < 250 = the chain streams ran concurrently with the caller's (own hardware queues),
        -1 = a chain shares a queue, 0 = not probed (one chain / no run yet)."""
        info = (ctypes.c_int32 * 9)()
        _lib.check(self.L.creg_train_plan_info(self.plan, info), "creg_train_plan_info")
        return int(info[8])

    def __del__(self):
        plan = getattr(self, "plan", None)
        if plan is not None and plan.value and ctypes is not None:      # (module globals may be gone at interpreter exit)
            self.L.creg_train_plan_destroy(plan)
            self.plan = None

    def _args(self, m, y, pts, offsets, params, lr, factor, patience, stop, outs):
        n = 6 if self.rot == 1 else 10
        if len(params) != n:
            raise ValueError(f"expected {n} parameter tensors, got {len(params)}")
        keep = [_need(m, torch.float32, "m"), _need(y, torch.float32, "y"), _need(pts, torch.float32, "pts"),
                _need(offsets, torch.int32, "offsets")]
        # the kernels index with the PLAN's sizes: a tensor of another shape would be read out of bounds, not rejected
        if tuple(keep[0].shape) != (self.k, 4, 4):
            raise ValueError(f"m must be ({self.k},4,4) for this plan, got {tuple(keep[0].shape)}")
        if tuple(keep[1].shape) != (self.n_tgt, 3):
            raise ValueError(f"y must be ({self.n_tgt},3) for this plan, got {tuple(keep[1].shape)}")
        if tuple(keep[2].shape) != (self.n_pred, 3):
            raise ValueError(f"pts must be ({self.n_pred},3) for this plan, got {tuple(keep[2].shape)}")
        if keep[3].numel() != self.k + 1:
            raise ValueError(f"offsets must hold {self.k + 1} entries, got {keep[3].numel()}")
        shapes_model = self._param_shapes(self.hidden_model)
        for p, want in zip(params, shapes_model):
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise TypeError("model parameters must be contiguous fp32 CUDA tensors")
            if p.numel() != int(np.prod(want)):
                raise ValueError(f"parameter tensor of {p.numel()} elements where the plan's model has {int(np.prod(want))}")
        self._padded = None
        if self.hidden_model != self.hidden:                                # zero-padded copies at the kernels' width (class docstring)
            padded = []
            for p, sm, sp in zip(params, shapes_model, self._param_shapes(self.hidden)):
                q = torch.zeros(sp, dtype=torch.float32, device=p.device)
                q[tuple(slice(0, d) for d in sm)] = p.view(sm)
                padded.append(q)
            self._padded = (padded, list(params), shapes_model)
            params = padded
        arr = (ctypes.c_void_p * n)(*[p.data_ptr() for p in params])
        self._keep = getattr(self, "_keep", [])[-64:] + [keep, arr, params]      # alive until the enqueued work has read them
        a = _lib.TrainArgs()
        a.m, a.y, a.local_pts, a.seg_offsets = [t.data_ptr() for t in keep]
        a.params = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
        a.lr, a.sched_factor, a.sched_patience, a.stop = lr, factor, patience, stop
        a.best_m, a.best_pred, a.loss_hist, a.lr_hist, a.result = [o.data_ptr() if o is not None else None for o in outs]
        return a

    def _param_shapes(self, H):
        """Shapes of the model's tensors in Q_PARAM_ORDER / DQ_PARAM_ORDER at width H (model_utils.py:65-168)."""
        if self.rot != 1:      # QRegMLP: enc 56->H, dec1 H->H/2->3, dec2 H->H->4; RRegMLP: 72 features, 6 outputs; RegMLP: 48, 3 (+ Tanh)
            nin, nout = _TWO_DECODER[self.rot]
            return [(H, nin), (H,), (H // 2, H), (H // 2,), (3, H // 2), (3,), (H, H), (H,), (nout, H), (nout,)]
        return [(H, 64), (H,), (H, H), (H,), (8, H), (8,)]        # DQRegMLP: enc 64->H, H->H, H->8

    def _param_numels(self):
        """Element counts of the model's tensors at the kernels' width."""
        return [int(np.prod(s)) for s in self._param_shapes(self.hidden)]

    def _unpad(self, padded):
        """Trained parameters back into the caller's tensors (stream-ordered copies of the leading blocks)."""
        if padded is not None:
            for q, p, sm in zip(*padded):
                p.view(sm).copy_(q[tuple(slice(0, d) for d in sm)])

    def _outs(self):
        dev = self.device
        return (torch.empty(self.k, 4, 4, dtype=torch.float32, device=dev),
                torch.empty(self.n_pred, 3, dtype=torch.float32, device=dev),
                torch.empty(self.epochs, dtype=torch.float32, device=dev),
                torch.empty(self.epochs, dtype=torch.float32, device=dev),
                torch.empty(4, dtype=torch.float32, device=dev))

    def run(self, m, y, pts, offsets, params, lr=2e-4, factor=0.7, patience=5, stop=200, same_target=False):
        """Returns (best_m (k,4,4), best_pred (n_pred,3), result (4) = [min_loss, epochs_run, lr,
        best_epoch], loss_hist (epochs), lr_hist (epochs)); all device tensors, stream-ordered."""
        return self.run_batch([(m, y, pts, offsets, params)], lr, factor, patience, stop, same_target)[0]

    def run_batch(self, problems, lr=2e-4, factor=0.7, patience=5, stop=200, same_target=False):
        """problems: list of `batch` tuples (m, y, pts, offsets, params) of identical shape, advanced
        together (one launch carries all of them).  Returns one result tuple per problem, as `run`.
        same_target: the caller vouches that every problem's `y` holds the values of this plan's previous run of that slot
        ("Anchor" after "Step" on the same frame, mlp_reg.py:338-356): the frame's k-d leaf blocks are kept instead of rebuilt."""
        if len(problems) != self.batch:
            raise ValueError(f"this plan advances {self.batch} problems per launch, got {len(problems)}")
        arr = (_lib.TrainArgs * self.batch)()
        outs, padded = [], []
        for b, (m, y, pts, offsets, params) in enumerate(problems):
            best_m, best_pred, lh, lrh, result = o = self._outs()
            arr[b] = self._args(m, y, pts, offsets, params, lr, factor, patience, stop, o)
            arr[b].y_unchanged = 1 if same_target else 0
            padded.append(self._padded)
            outs.append((best_m, best_pred, result, lh, lrh))
        _lib.check(self.L.creg_train_plan_run_batch(self.plan, arr, self.batch, _stream()), "creg_train_plan_run_batch")
        for pd in padded:
            self._unpad(pd)
        return outs

    #: scalar fields of a train's control state (creg_train_state; `state_out` of creg_train_plan_resume holds them in this order + last_loss)
    STATE_FIELDS = ("step", "epochs_run", "lr", "sched_best", "sched_bad", "count", "min_loss", "best_epoch", "stopped")

    def resume(self, m, y, pts, offsets, params, state, n_epochs=1, factor=0.7, patience=5, stop=200, best=None):
        """`n_epochs` further epochs of one train from a caller-supplied optimizer / control state (creg_train_plan_resume): checkpoint /
        resume, and the teacher-forced parity hook.  `state`: dict with `exp_avg`, `exp_avg_sq` (lists of fp32 CUDA tensors shaped like
        `params`: torch.optim.Adam's moments) and the scalars of STATE_FIELDS (missing ones default to a fresh train's).  `best`:
        (best_m (k,4,4), best_pred (n_pred,3)) so far, required when state['best_epoch'] >= 0.  `params` are updated in place.
        Returns (best_m, best_pred, result, loss_hist, lr_hist, state_after) -- state_after like `state`, its scalars read back
        (synchronises the stream for them)."""
        if self.hidden_model != self.hidden:
            raise ValueError("resume needs the model at one of the kernels' widths (64, 128, 256, 512): no zero-padding of the moments")
        n = 6 if self.rot == 1 else 10
        ea, es = list(state["exp_avg"]), list(state["exp_avg_sq"])
        if len(ea) != n or len(es) != n:
            raise ValueError(f"expected {n} moment tensors of each kind")
        for q, p in zip(ea + es, list(params) * 2):
            if not (q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.numel() == p.numel()):
                raise TypeError("Adam moments must be contiguous fp32 CUDA tensors shaped like the parameters")
        o = self._outs()
        best_epoch = int(state.get("best_epoch", -1))
        if best_epoch >= 0:
            if best is None:
                raise ValueError("state['best_epoch'] >= 0 needs best=(best_m, best_pred)")
            o[0].copy_(best[0]); o[1].copy_(best[1])
        a = self._args(m, y, pts, offsets, params, float(state.get("lr", 2e-4)), factor, patience, stop, o)
        st = _lib.TrainState()
        arr_a = (ctypes.c_void_p * n)(*[q.data_ptr() for q in ea])
        arr_s = (ctypes.c_void_p * n)(*[q.data_ptr() for q in es])
        st.exp_avg, st.exp_avg_sq = ctypes.cast(arr_a, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(arr_s, ctypes.POINTER(ctypes.c_void_p))
        st.lr, st.sched_best = float(state.get("lr", 2e-4)), float(state.get("sched_best", float("inf")))
        st.step, st.epochs_run = int(state.get("step", 0)), int(state.get("epochs_run", state.get("step", 0)))
        st.sched_bad, st.count, st.best_epoch, st.stopped = int(state.get("sched_bad", 0)), int(state.get("count", 0)), best_epoch, int(state.get("stopped", 0))
        st.min_loss = float(state.get("min_loss", 1000.0))
        ea2, es2 = [torch.empty_like(q) for q in ea], [torch.empty_like(q) for q in es]
        out_a = (ctypes.c_void_p * n)(*[q.data_ptr() for q in ea2])
        out_s = (ctypes.c_void_p * n)(*[q.data_ptr() for q in es2])
        sc = torch.empty(12, dtype=torch.float64, device=self.device)
        _lib.check(self.L.creg_train_plan_resume(self.plan, ctypes.byref(a), ctypes.byref(st), int(n_epochs),
                                                 ctypes.cast(out_a, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(out_s, ctypes.POINTER(ctypes.c_void_p)),
                                                 _p(sc), _stream()), "creg_train_plan_resume")
        h = sc.cpu().tolist()
        after = {"exp_avg": ea2, "exp_avg_sq": es2, "last_loss": h[9]}
        for i, k in enumerate(self.STATE_FIELDS):
            after[k] = h[i] if k in ("lr", "sched_best", "min_loss") else int(h[i])
        return o[0], o[1], o[4], o[2], o[3], after

    def probe(self, m, y, pts, offsets, params):
        """One forward + pose-gradient evaluation (test hook): (m2, pred, loss, grad_m2)."""
        dev = self.device
        m2 = torch.empty(self.k, 4, 4, dtype=torch.float32, device=dev)
        pred = torch.empty(self.n_pred, 3, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        gm = torch.empty(self.k, 4, 4, dtype=torch.float32, device=dev)
        a = self._args(m, y, pts, offsets, params, 2e-4, 0.7, 5, 200, (None, None, None, None, None))
        _lib.check(self.L.creg_train_plan_probe(self.plan, ctypes.byref(a), _p(m2), _p(pred), _p(loss), _p(gm),
                                                _stream()), "creg_train_plan_probe")
        return m2, pred, loss, gm

    KERNELS = ("_", "head", "nn_l1", "gradc", "bd", "l2")

    def profile(self, m, y, pts, offsets, params, n_epochs=50):
        """Average event-bracketed microseconds of each of the 5 epoch kernels, and the back-to-back launch time of each
        (synchronises; the plan's copy of the parameters moves on, the caller's tensors are not written)."""
        out = (ctypes.c_float * 16)()
        a = self._args(m, y, pts, offsets, params, 2e-4, 0.7, 5, 200, (None, None, None, None, None))
        _lib.check(self.L.creg_train_plan_profile(self.plan, ctypes.byref(a), n_epochs, out, _stream()),
                   "creg_train_plan_profile")
        d = dict(zip(self.KERNELS, [float(v) for v in out]))
        d.pop("_")
        d["nn_l1_back_to_back"] = float(out[6])
        d["nn_l1_problems_per_launch"] = int(out[7])
        d["bd_back_to_back"] = float(out[8])
        d["l2_back_to_back"] = float(out[9])
        d["head_back_to_back"] = float(out[10])
        d["gradc_back_to_back"] = float(out[11])
        return d
