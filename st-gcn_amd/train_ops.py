"""The training-step ops around the block stack on the HIP library (SURVEY.md
§8(f) row 1): the classification head (global average pool over (T, V) +
Linear + cross entropy; lightning_model.py:105-107 and the loss of
training_step :202) as one autograd Function, and ``FusedAdam``, a drop-in for
``torch.optim.Adam`` (lightning_model.py:196-197) whose step is ONE kernel
launch over every parameter (same hyper-parameters, same per-parameter state
names ``step`` / ``exp_avg`` / ``exp_avg_sq``, so state_dicts interchange),
with ``FusedAdamW`` and AMSGrad beside it.
No CPU fallback: both raise without the HIP library / a GPU.
"""
import ctypes

import torch

from . import hip_lib


def _check_f32(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a contiguous float32 GPU tensor")


class StgcnHeadFn(torch.autograd.Function):
    """forward(y (N,C,T,V), W (classes,C), b (classes), labels int64 (N)) ->
    (loss (scalar, mean cross entropy), logits (N, classes), non-differentiable).
    Same arithmetic as ``F.cross_entropy(fc_layer(avg_pool2d(y, (T,V)).view(N,C)), labels)``.
    from_u = (U, stats2, g2, b2) (ABI 9, model.STGCNStack.forward_loss): y is the
    last block's UNWRITTEN output; the pool forms y = ReLU(BN2(U)) on load
    (stgcn_head_fwd_u, bit-identical); y still receives the gradient."""

    @staticmethod
    def forward(ctx, y, W, b, labels, from_u=None):
        lib = hip_lib.lib()
        if from_u is None:
            y = y.contiguous()
            _check_f32(y, "y")
        # (from_u: y is the block's unwritten output, a shape-only placeholder)
        for t, n in ((W, "W"), (b, "b")):
            _check_f32(t, n)
        if labels.dtype != torch.int64 or not labels.is_cuda:
            raise RuntimeError("labels: expected an int64 GPU tensor")
        labels = labels.contiguous()
        N, C = y.shape[0], y.shape[1]
        L = y[0, 0].numel()
        classes = W.shape[0]
        if W.shape[1] != C or b.shape[0] != classes or labels.shape[0] != N:
            raise RuntimeError("head: shape mismatch between y, W, b and labels")
        d = hip_lib.HeadDesc(N, C, L, classes)
        dev = y.device
        pooled = torch.empty((N, C), device=dev, dtype=torch.float32)
        logits = torch.empty((N, classes), device=dev, dtype=torch.float32)
        lossv = torch.empty(N, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        if from_u is not None:
            U, stats2, g2, b2 = from_u
            for t, n in ((U, "U"), (stats2, "stats2"), (g2, "g2"), (b2, "b2")):
                _check_f32(t, n)
            if U.shape != y.shape or stats2.numel() < 2 * C or g2.numel() != C or b2.numel() != C:
                raise RuntimeError("head: U / BN2 parameters do not match y")
            hip_lib.check(lib.stgcn_head_fwd_u(ctypes.byref(d), *[hip_lib.ptr(t) for t in (
                U, stats2, g2, b2, W, b, labels, pooled, logits, lossv, loss)],
                hip_lib.stream_handle(dev)))
        else:
            hip_lib.check(lib.stgcn_head_fwd(ctypes.byref(d), *[hip_lib.ptr(t) for t in (
                y, W, b, labels, pooled, logits, lossv, loss)], hip_lib.stream_handle(dev)))
        ctx.save_for_backward(pooled, logits, W, labels)
        ctx.shape = y.shape
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        lib = hip_lib.lib()
        pooled, logits, W, labels = ctx.saved_tensors
        N, C = pooled.shape
        classes = W.shape[0]
        dev = pooled.device
        L = 1
        for s in ctx.shape[2:]:
            L *= s
        d = hip_lib.HeadDesc(N, C, L, classes)
        dloss = dloss.reshape(1).float().contiguous()
        dlogits = torch.empty((N, classes), device=dev, dtype=torch.float32)
        dpooled = torch.empty((N, C), device=dev, dtype=torch.float32)
        dW = torch.empty_like(W)
        db = torch.empty(classes, device=dev, dtype=torch.float32)
        # ABI 10: the pool's gradient is constant over (T, V): only its value per
        # (n, c) is formed, returned as that (N, C) tensor expanded (stride 0) to
        # y's shape. A HIP block takes it as stgcn_bwd_args_t.dy_nc (no dy tensor
        # written or read); any other consumer materialises it (.contiguous()).
        dy_nc = torch.empty((N, C), device=dev, dtype=torch.float32)
        hip_lib.check(lib.stgcn_head_bwd_nc(ctypes.byref(d), *[hip_lib.ptr(t) for t in (
            pooled, logits, W, labels, dloss, dlogits, dpooled, dy_nc, dW, db)],
            hip_lib.stream_handle(dev)))
        dy = dy_nc.view(N, C, *([1] * (len(ctx.shape) - 2))).expand(ctx.shape)
        return dy, dW, db, None, None


def decode_eval_metrics(buf, classes):
    """The dict of a metrics block (stgcn_hip.h, stgcn_head_eval): ``buf`` its
    bytes as a CPU uint8 tensor. batches, clips (with a valid label), invalid,
    correct, topk_hits; loss / acc / topk_acc per clip; val_loss / val_acc the
    mean of the batch means (validation_epoch_end, lightning_model.py:220-224,
    which differs from the per-clip mean when the last batch is short);
    confusion[label][pred] (int64, classes x classes; compute_conf_mat :123-133).
    Pure host code: no GPU, no library."""
    head = hip_lib.METRICS_WORDS * 8
    nbytes = head + 8 * classes * classes
    if buf.dtype != torch.uint8 or buf.is_cuda or buf.numel() != nbytes:
        raise ValueError(f"metrics block: expected {nbytes} CPU uint8 bytes for {classes} classes")
    buf = buf.contiguous().clone()
    ints = buf[:head].view(torch.int64).tolist()
    dbls = buf[:head].view(torch.float64).tolist()
    batches, clips, correct, hits, invalid = ints[:5]
    sum_loss, sum_batch_loss, sum_batch_acc = dbls[5:8]

    def over(a, b):
        return a / b if b else 0.0

    return {"batches": batches, "clips": clips, "invalid": invalid, "correct": correct,
            "topk_hits": hits, "loss": over(sum_loss, clips), "acc": over(correct, clips),
            "topk_acc": over(hits, clips), "val_loss": over(sum_batch_loss, batches),
            "val_acc": over(sum_batch_acc, batches),
            "confusion": buf[head:].view(torch.int64).reshape(classes, classes).clone()}


class EvalMetrics:
    """The metrics of an evaluation epoch, accumulated on the device by
    ``head_eval`` (stgcn_head_eval): counts, loss and accuracy sums and the
    confusion matrix. No host read until ``result()``, which makes one
    device-to-host copy, so an evaluation step can be captured in a HIP graph
    (``GraphedStep``). ``topk``: the k of the top-k hit count."""

    def __init__(self, classes, topk=1, device="cuda", buf=None):
        """buf: a caller's uint8 device tensor of stgcn_eval_metrics_bytes(classes)
        bytes to use as the block (reset here like an own one)."""
        lib = hip_lib.lib()
        nbytes = lib.stgcn_eval_metrics_bytes(int(classes))
        if not nbytes:
            raise ValueError(f"EvalMetrics: unsupported number of classes {classes}")
        if not 1 <= topk <= classes:
            raise ValueError("EvalMetrics: topk must be in [1, classes]")
        self.classes, self.topk = int(classes), int(topk)
        if buf is None:
            buf = torch.empty(nbytes, device=device, dtype=torch.uint8)
        elif (buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous()
              or buf.numel() != nbytes or buf.data_ptr() % 8):
            raise ValueError(f"EvalMetrics: buf must be {nbytes} contiguous, 8-byte aligned "
                             "uint8 bytes on the GPU")
        self.buf = buf
        self.reset()

    def reset(self):
        hip_lib.check(hip_lib.lib().stgcn_eval_metrics_reset(
            hip_lib.ptr(self.buf), self.classes, hip_lib.stream_handle(self.buf.device)))

    def result(self):
        return decode_eval_metrics(self.buf.cpu(), self.classes)


def _loss_options(weight, label_smoothing, classes, dev):
    """Validate F.cross_entropy's ``weight`` / ``label_smoothing`` for a head of
    ``classes`` classes on ``dev``; returns label_smoothing as a float."""
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)):
        raise ValueError("label_smoothing: expected a float in [0, 1]")
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:  # (NaN fails both comparisons)
        raise ValueError(f"label_smoothing: expected a float in [0, 1], got {label_smoothing}")
    if weight is not None:
        if not torch.is_tensor(weight):
            raise ValueError("weight: expected a tensor of one float32 per class")
        if weight.dim() != 1 or weight.shape[0] != classes:
            raise ValueError(f"weight: expected {classes} elements (one per class), got "
                             f"shape {tuple(weight.shape)}")
        _check_f32(weight, "weight")
        if weight.device != dev:
            raise RuntimeError(f"weight: on {weight.device}, the head runs on {dev}")
    return eps


def head_eval(y, W, b, labels, topk=1, metrics=None, from_u=None, weight=None,
              label_smoothing=0.0):
    """The head of an evaluation step (stgcn_head_eval_loss / _u): y
    (N, C, T, V), W (classes, C), b (classes), labels int64 (N) -> (loss, logits
    (N, classes), pred int32 (N), lossv (N) the per-clip losses), with ``StgcnHeadFn``'s logits and loss bit for
    bit when every label is valid; a label outside [0, classes) is ignored as
    F.cross_entropy's ignore_index. metrics: an ``EvalMetrics`` that takes the
    batch (its topk then applies). from_u = (U, stats2, g2, b2): y is None and the
    pool forms ReLU(BN2(U)) on load. No autograd, no host read.
    weight (contiguous float32 GPU tensor, one element per class, on y's device)
    / label_smoothing: F.cross_entropy's: loss is the sum of the per-clip losses
    over D = the valid clips' summed w[label], and 0 (torch: NaN) when D == 0.
    Every call goes through stgcn_head_eval_loss / _u (without options: flags 0,
    eps 0, which has stgcn_head_eval's bits)."""
    lib = hip_lib.lib()
    src = y if from_u is None else from_u[0]
    if from_u is None:
        src = src.contiguous()
    for t, n in ((src, "y" if from_u is None else "U"), (W, "W"), (b, "b")):
        _check_f32(t, n)
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise RuntimeError("labels: expected an int64 GPU tensor")
    labels = labels.contiguous()
    N, C = src.shape[0], src.shape[1]
    L = src[0, 0].numel()
    classes = W.shape[0]
    if W.shape[1] != C or b.shape[0] != classes or labels.shape[0] != N:
        raise RuntimeError("head: shape mismatch between y, W, b and labels")
    mbuf = None
    if metrics is not None:
        if metrics.classes != classes or metrics.buf.device != src.device:
            raise RuntimeError("head: the metrics block is for other classes or another device")
        topk, mbuf = metrics.topk, metrics.buf
    dev = src.device
    eps = _loss_options(weight, label_smoothing, classes, dev)
    d = hip_lib.LossDesc(N, C, L, classes, int(topk),
                         hip_lib.LOSS_WEIGHT if weight is not None else 0, eps)
    hip_lib.check(lib.stgcn_loss_check(ctypes.byref(d)))
    pooled = torch.empty((N, C), device=dev, dtype=torch.float32)
    logits = torch.empty((N, classes), device=dev, dtype=torch.float32)
    lossv = torch.empty(N, device=dev, dtype=torch.float32)
    denom = torch.empty((), device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    pred = torch.empty(N, device=dev, dtype=torch.int32)
    rest = (W, b, weight, labels, pooled, logits, lossv, denom, loss, pred, mbuf)
    if from_u is not None:
        U, stats2, g2, b2 = from_u
        for t, n in ((stats2, "stats2"), (g2, "g2"), (b2, "b2")):
            _check_f32(t, n)
        if stats2.numel() < 2 * C or g2.numel() != C or b2.numel() != C:
            raise RuntimeError("head: BN2 parameters do not match U")
        hip_lib.check(lib.stgcn_head_eval_loss_u(ctypes.byref(d), *[hip_lib.ptr(t) for t in (
            U, stats2, g2, b2) + rest], hip_lib.stream_handle(dev)))
    else:
        hip_lib.check(lib.stgcn_head_eval_loss(ctypes.byref(d), *[hip_lib.ptr(t) for t in (
            src,) + rest], hip_lib.stream_handle(dev)))
    return loss, logits, pred, lossv


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (maximize=False, fp32 parameters on one
    device) with the update as one libstgcn_hip launch per step. The tensor
    table (pointers of param / grad / exp_avg / exp_avg_sq) is rebuilt on the
    host only when a pointer changed (e.g. grads re-allocated after
    zero_grad(set_to_none=True)) and copied to the device asynchronously from
    pinned memory; one table per parameter group (keyed by the group's index).

    capturable=True (as torch.optim.Adam(capturable=True)): the step count lives
    on the device (one float tensor per group, shared by the group's parameters'
    ``state["step"]``) and is advanced by the library (stgcn_opt_step's
    step_dev), so ``step()`` reads nothing from the device and can be captured in a HIP
    graph (``GraphedStep``). A table built during a capture (the captured
    backward allocates new gradients) is written into a pinned buffer set aside
    by the last eager build and kept alive with the table: every replay's copy
    re-reads it.

    lr as a tensor (capturable=True only): a 0-dim float32 tensor on the
    parameters' device is read by the kernel when it runs (stgcn_opt_step's lr_dev),
    so a scheduler that writes it with ``fill_`` between replays (torch's
    lr_scheduler does for a tensor lr) takes effect without a re-capture. Any
    other tensor raises; a float lr takes the by-value call as before.

    max_grad_norm (capturable=True only): the 2-norm of all gradients of all
    groups is formed on the device (stgcn_grad_norm: fixed-order fp64 sums, no
    atomics, the same bits every run) and the step uses g * clip_coef with
    clip_coef = min(1, max_grad_norm / (norm + 1e-6)), the coefficient of
    ``torch.nn.utils.clip_grad_norm_``, applied before the weight-decay term as
    when clip_grad_norm_ runs before step(). ``opt.grad_norm`` and
    ``opt.clip_coef`` are the device tensors of the last step. Unlike
    clip_grad_norm_, ``p.grad`` itself is NOT rescaled: code that reads the
    gradients after the step sees the unclipped ones. Under data parallelism the
    step runs after the all-reduce, so the norm is the global one.

    amsgrad / decoupled_weight_decay (per group, as torch.optim.Adam's): the same
    arithmetic with p = p * (1 - lr * wd) in place of the gradient's decay term
    (torch.optim.AdamW) and / or the running maximum ``max_exp_avg_sq`` in the
    denominator, in every launch form above. Every group steps through
    stgcn_opt_step, whose stgcn_opt_check refuses a negative lr / eps /
    weight_decay and betas outside [0, 1) (as torch.optim.Adam's constructor)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, capturable=False, max_grad_norm=None,
                 decoupled_weight_decay=False):
        if max_grad_norm is not None:
            if not capturable:
                raise ValueError("FusedAdam: max_grad_norm needs capturable=True")
            if not float(max_grad_norm) > 0:
                raise ValueError("FusedAdam: max_grad_norm must be positive")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      amsgrad=bool(amsgrad),
                                      decoupled_weight_decay=bool(decoupled_weight_decay)))
        self.capturable = capturable
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = self.clip_coef = None  # device tensors (max_grad_norm)
        self._norm_partials = None
        self._lr_dev = {}  # group index -> (value, device float) of a float lr (clipping)
        self._tables = {}  # group index -> (key, device table, chunks, ntensors, host table)
        self._spare = {}   # group index -> unused pinned table buffer (capturable)
        self._captured = []  # pinned tables a captured step's copies read

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = hip_lib.lib()
        coef = self._clip() if self.max_grad_norm is not None else None
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group["params"] if p.grad is not None]
            if not plist:
                continue
            for p in plist:
                _check_f32(p, "param")
                _check_f32(p.grad, "grad")
            lr = group["lr"]
            if torch.is_tensor(lr):
                if not (self.capturable and lr.dim() == 0 and lr.dtype == torch.float32
                        and lr.device == plist[0].device):
                    raise RuntimeError(
                        "FusedAdam: a tensor lr must be a 0-dim float32 tensor on the "
                        "parameters' device, with capturable=True")
            if self.capturable:
                dstep = self._device_step(plist)
            else:
                for p in plist:
                    st = self.state[p]
                    if not st:
                        st["step"] = torch.tensor(0.0)
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["step"] = st["step"] + 1  # (not in place: loaded state may share it)
                steps = {int(self.state[p]["step"].item()) for p in plist}
                if len(steps) != 1:
                    raise RuntimeError("FusedAdam: parameters of a group at different steps")
                step = steps.pop()
            dev = plist[0].device
            amsgrad = bool(group.get("amsgrad", False))
            decoupled = bool(group.get("decoupled_weight_decay", False))
            if coef is not None and not torch.is_tensor(lr) and not (amsgrad or decoupled):
                # (a float lr next to clipping, on a group with neither option, is
                # rounded to float32; DESIGN.md "Optimizers" records the asymmetry)
                lr = self._lr_tensor(gi, lr, dev)
            tabs = []
            for p in plist:
                st = self.state[p]
                vmax = None
                if amsgrad:
                    if "max_exp_avg_sq" not in st:
                        if torch.cuda.is_current_stream_capturing():
                            raise RuntimeError("FusedAdam: capture a step only after an eager "
                                               "step of the same parameters (GraphedStep warm-up)")
                        st["max_exp_avg_sq"] = torch.zeros_like(
                            p, memory_format=torch.preserve_format)
                    vmax = st["max_exp_avg_sq"]
                    _check_f32(vmax, "max_exp_avg_sq")
                tabs.append(hip_lib.OptTensor(
                    p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                    st["exp_avg_sq"].data_ptr(), None if vmax is None else vmax.data_ptr(),
                    p.numel(), 0, 0))
            b1, b2 = group["betas"]
            flags = (hip_lib.OPT_AMSGRAD if amsgrad else 0) | \
                (hip_lib.OPT_DECOUPLED_WD if decoupled else 0)
            desc = hip_lib.OptDesc(
                hip_lib.OPT_ADAM, flags, 0.0 if torch.is_tensor(lr) else float(lr), b1, b2,
                group["eps"], group["weight_decay"], 0 if self.capturable else step,
                hip_lib.ptr(lr) if torch.is_tensor(lr) else None, hip_lib.ptr(coef),
                hip_lib.ptr(dstep) if self.capturable else None)
            _, dev_table, nchunks, n, _ = self._table(
                gi, hip_lib.OptTensor, tabs, lib.stgcn_opt_table_bytes,
                lambda *a: lib.stgcn_opt_build_table(ctypes.byref(desc), *a), dev)
            hip_lib.check(lib.stgcn_opt_step(
                ctypes.byref(desc), hip_lib.ptr(dev_table), n, nchunks,
                hip_lib.stream_handle(dev)))
        return loss

    def _table(self, gi, entry, tabs, table_bytes, build, dev):
        """(key, device table, chunks, ntensors, host table) of the ``entry``
        structs ``tabs`` (hip_lib.OptTensor for a step, hip_lib.AdamTensor for the
        gradient norm), cached under ``gi`` and rebuilt when a field changed.
        table_bytes(n) / build(array, n, host pointer, bytes, chunks out): the
        library's pair for that entry type."""
        names = [f for f, _ in entry._fields_]
        key = (entry,) + tuple(tuple(getattr(t, f) for f in names) for t in tabs)
        cached = self._tables.get(gi)
        if cached is None or cached[0] != key:
            n = len(tabs)
            nbytes = table_bytes(n)
            if torch.cuda.is_current_stream_capturing():
                # (no pinned allocation inside a capture: the spare buffer
                # the last eager build left, never yet read by a copy)
                host = self._spare.pop(gi, None)
                if host is None or host.numel() < nbytes:
                    raise RuntimeError("FusedAdam: capture a step only after an eager "
                                       "step of the same parameters (GraphedStep warm-up)")
                self._captured.append(host)  # (read by every replay: never freed)
            else:
                host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                if self.capturable:
                    self._spare[gi] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            chunks = ctypes.c_int64(0)
            hip_lib.check(build((entry * n)(*tabs), n, ctypes.c_void_p(host.data_ptr()), nbytes,
                                ctypes.byref(chunks)))
            dev_table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dev_table.copy_(host, non_blocking=True)
            cached = (key, dev_table, chunks.value, n, host)
            self._tables[gi] = cached
        return cached

    def _lr_tensor(self, gi, lr, dev):
        """A float lr as a device word (the clipped step of a group with neither
        amsgrad nor decoupled decay; the value rounded to float32, as a tensor lr is):
        rewritten when the value changes; inside a capture the write is part of
        the graph, so a captured step keeps its capture's value, like the
        by-value call."""
        held = self._lr_dev.get(gi)
        if held is None or held[0] != float(lr):
            held = (float(lr), torch.full((), float(lr), device=dev, dtype=torch.float32))
            self._lr_dev[gi] = held
        return held[1]

    def _clip(self):
        """The global gradient norm and clip coefficient of this step on the
        device (one table over every group's tensors); returns clip_coef."""
        lib = hip_lib.lib()
        plist = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not plist:
            return None
        for p in plist:
            _check_f32(p, "param")
            _check_f32(p.grad, "grad")
        for g in self.param_groups:  # (the table carries the state pointers: create them)
            gp = [p for p in g["params"] if p.grad is not None]
            if gp:
                self._device_step(gp)
        dev = plist[0].device
        tabs = [hip_lib.AdamTensor(p.data_ptr(), p.grad.data_ptr(),
                                   self.state[p]["exp_avg"].data_ptr(),
                                   self.state[p]["exp_avg_sq"].data_ptr(), p.numel())
                for p in plist]
        _, dev_table, nchunks, n, _ = self._table(
            "norm", hip_lib.AdamTensor, tabs, lib.stgcn_adam_table_bytes,
            lib.stgcn_adam_build_table, dev)
        if self.grad_norm is None:
            self.grad_norm = torch.zeros((), device=dev, dtype=torch.float32)
            self.clip_coef = torch.ones((), device=dev, dtype=torch.float32)
        need = lib.stgcn_grad_norm_bytes(nchunks) // 8
        if self._norm_partials is None or self._norm_partials.numel() < need:
            if torch.cuda.is_current_stream_capturing() and self._norm_partials is not None:
                raise RuntimeError("FusedAdam: the parameter set grew inside a capture")
            self._norm_partials = torch.empty(need, device=dev, dtype=torch.float64)
        hip_lib.check(lib.stgcn_grad_norm(
            hip_lib.ptr(dev_table), n, nchunks, self.max_grad_norm,
            hip_lib.ptr(self._norm_partials), hip_lib.ptr(self.grad_norm),
            hip_lib.ptr(self.clip_coef), hip_lib.stream_handle(dev)))
        return self.clip_coef

    def _device_step(self, plist):
        """The group's device step count (float32, shape ()): created with the
        state (0), or taken over from loaded state once (one host read, outside
        any capture), then shared by every parameter of the group."""
        dev = plist[0].device
        shared = None
        for p in plist:
            st = self.state[p].get("step")
            if torch.is_tensor(st) and st.is_cuda and st.dtype == torch.float32 and st.dim() == 0:
                shared = st if shared is None else shared
        if shared is None or any(self.state[p].get("step") is not shared for p in plist):
            vals = {float(self.state[p]["step"]) for p in plist if "step" in self.state[p]}
            if len(vals) > 1:
                raise RuntimeError("FusedAdam: parameters of a group at different steps")
            shared = torch.full((), vals.pop() if vals else 0.0, device=dev, dtype=torch.float32)
            for p in plist:
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = shared
        return shared


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: FusedAdam with decoupled weight decay (default 1e-2)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 amsgrad=False, capturable=False, max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         amsgrad=amsgrad, capturable=capturable, max_grad_norm=max_grad_norm,
                         decoupled_weight_decay=True)


class GraphedStep:
    """One training step captured in a HIP graph and replayed (torch.cuda.graph
    over the caller's stream work: every libstgcn_hip launch goes to the capture
    stream, allocations come from the graph's private pool, so replays reuse the
    same buffers). ``step_fn()`` must be replay-safe: static inputs (copy new
    data into them before ``__call__``), no host reads of device values,
    optimizer ``FusedAdam(capturable=True)``. Per-step values come from device
    memory: dropout needs ``STGCNStack(dropout_seed="device")`` (a host seed
    raises at capture), a learning-rate schedule a tensor ``lr``, clipping
    ``FusedAdam(max_grad_norm=...)``. ``warmup`` eager calls run first on a side stream (the torch
    recipe: lazy allocations and table builds happen outside the capture).
    ``__call__`` replays and returns the tensors the captured call returned
    (their storage is rewritten by every replay)."""

    def __init__(self, step_fn, warmup=3):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step_fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()  # (the warm-up's host-to-device table copies have run)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = step_fn()

    def __call__(self):
        self.graph.replay()
        return self.out


class GraphedDPStep:
    """The multi-rank training step in two HIP graphs around an eager gradient
    all-reduce: graph A = ``dp.zero_grad()`` + ``fwd_bwd()`` under
    ``dp.no_sync()`` (the gradients accumulate into the bucket views,
    dp.GradAllReduce, and no collective is issued inside the capture), then
    ``dp.synchronize()`` eagerly (one all-reduce per bucket + the division by
    the world size), then graph B = ``opt_step()`` (FusedAdam(capturable=True)).
    The collectives stay outside the graphs, so the path is the same for RCCL and
    gloo; what is given up against the eager step is the overlap of the bucket
    all-reduces with backward (~11 MB per step: a small fraction of the step on
    xGMI), what is gained is the per-launch host work of ~220 launches. The
    result equals the eager DP step's: the same gradients reach the same
    all-reduce of each bucket (tests/dp_graph_worker.py). ``warmup`` full eager
    steps run first on a side stream (lazy allocations, Adam state, tables)."""

    def __init__(self, fwd_bwd, dp, opt_step, warmup=2):
        self.dp = dp

        def a():
            dp.zero_grad()
            with dp.no_sync():
                return fwd_bwd()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                a()
                dp.synchronize()
                opt_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph_a = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_a):
            self.out = a()
        self.graph_b = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_b):
            opt_step()

    def __call__(self):
        self.graph_a.replay()
        self.dp.synchronize()
        self.graph_b.replay()
        return self.out
