"""Optimizer step of the reference trainer on the MI355X.

`AdamW` keeps the constructor, state keys (`step`, `exp_avg`, `exp_avg_sq`) and arithmetic of data/utils/build_optimizer.py:105-197
(decoupled weight decay applied after the Adam update, eps 1e-6 added to sqrt(v), optional bias correction), so optimizer
checkpoints interchange.  `step()` is ONE kernel launch per (parameter group, step count): a multi-tensor pass over a descriptor
table (mico_adamw_step), which also refreshes the 16-bit GEMM-operand mirrors of the weights the engine caches
(runtime.gemm_weight) - no re-cast pass follows an optimizer step.  `build_optimizer` reproduces the reference's grouping
(:11-76): basic / new / CLIP-visual parameters, each with and without weight decay.

Global-norm gradient clipping (`AdamW(max_grad_norm=...)`, `clip_grad_norm_`; the reference carries the knob - data/utils/args.py:230
--grad_norm, data/utils/pipeline.py:102-103 - with the call commented out) costs no pass of its own over the gradients and no host read: the
sum of squares comes out of the pass that checks them for inf / NaN (mico_grad_sumsq), the coefficient stays in device memory
(mico_grad_clip_coef) and the update kernel reads it from there (mico_adamw_step_dev)."""
import ctypes as C
import math

import torch

from . import _lib, runtime

CHUNK = 1 << 16
_FROM_ATTRIBUTE = object()      # AdamW.step(max_grad_norm=...) default: the optimizer's own attribute
_chunk_cache = {}


def _chunk_lists(numels, dev, cache=_chunk_cache):
    """(chunk_tensor int32, chunk_start int64, nchunks) on `dev`: the tensors of a descriptor table cut into pieces of CHUNK elements"""
    key = (tuple(numels), str(dev))
    hit = cache.get(key)
    if hit is None:
        ct, cs = [], []
        for t, n in enumerate(numels):
            for s in range(0, n, CHUNK):
                ct.append(t)
                cs.append(s)
        hit = (torch.tensor(ct, dtype=torch.int32).to(dev), torch.tensor(cs, dtype=torch.int64).to(dev), len(ct))
        cache[key] = hit
    return hit


def _check_max_norm(max_norm):
    if not float(max_norm) > 0.0:
        raise ValueError("Invalid max_grad_norm: {} - should be > 0 (None: no clipping)".format(max_norm))
    return float(max_norm)


def _fp32(g):
    return g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()


def _grad_table(grads, cache=_chunk_cache):
    """descriptor table (.g / .numel only) + chunk lists over fp32 contiguous device gradients"""
    dev = grads[0].device
    descs = (_Desc * len(grads))()
    for d, g in zip(descs, grads):
        if not g.is_cuda:
            raise _lib.MicoHipError("mico_amd.optim reads device gradients only (no CPU path)")
        assert g.device == dev and g.dtype == torch.float32 and g.is_contiguous()
        d.g, d.numel = g.data_ptr(), g.numel()
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    return table, _chunk_lists([g.numel() for g in grads], dev, cache)


def _grad_norm_coef(grads, max_norm, grad_mult=1.0, flag=None, cache=_chunk_cache):
    """(total_norm, coef), fp32 device scalars, of the fp32 contiguous gradients `grads` times grad_mult: one mico_grad_sumsq launch (which also
    sets `flag` on an inf / NaN, as mico_grads_finite would) and one mico_grad_clip_coef launch on the current stream.  No host read."""
    lib = _lib.lib()
    dev = grads[0].device
    stream = torch.cuda.current_stream(dev).cuda_stream
    table, (ct, cs, n) = _grad_table(grads, cache)
    sumsq = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.check(lib.mico_grad_sumsq(table.data_ptr(), len(grads), ct.data_ptr(), cs.data_ptr(), n, CHUNK, float(grad_mult), sumsq.data_ptr(),
                                   None if flag is None else flag.data_ptr(), stream), "mico_grad_sumsq")
    _lib.check(lib.mico_grad_clip_coef(sumsq.data_ptr(), n, float(max_norm), out.data_ptr(), out.data_ptr() + 4, stream), "mico_grad_clip_coef")
    return out[0], out[1]


class _Desc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_int64),
                ("w16", C.c_void_p), ("ld16", C.c_int64), ("lo_off", C.c_int64), ("cols", C.c_int), ("w16_dtype", C.c_int)]


class AdamW(torch.optim.Optimizer):
    """max_grad_norm (None: off): clip the gradients of ALL param groups to this global 2-norm inside step(), with the semantics of
    torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False): coef = min(1, max_norm / (total_norm + 1e-6)), the update uses
    g * (grad_mult * coef).  It is an attribute of the optimizer, not a param-group key and not part of state_dict(): optimizer checkpoints keep
    interchanging with the reference's.  `last_grad_norm` is the fp32 device scalar of the last clipped step (of the un-scaled gradients; None
    before the first one) - read it for logging whenever a host sync is acceptable.
    Data parallel: step() runs after GradBucketReducer.finish(), when every rank holds the same averaged gradients, so every rank computes the
    same norm from the same bits in the same order - clipping adds no collective."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        if max_grad_norm is not None:
            _check_max_norm(max_grad_norm)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self._chunk_cache = {}
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None

    def _chunks(self, numels, dev):
        return _chunk_lists(numels, dev, self._chunk_cache)

    def _grads(self):
        """every gradient this optimizer would consume (all groups), as fp32 contiguous tensors"""
        return [_fp32(p.grad) for group in self.param_groups for p in group["params"] if p.grad is not None]

    @torch.no_grad()
    def grads_nonfinite(self, flag):
        """flag (fp32 device scalar) <- 1 if any gradient this optimizer would consume is inf / NaN; no host sync here."""
        grads = self._grads()
        if not grads:
            return flag
        table, (ct, cs, n) = _grad_table(grads, self._chunk_cache)
        _lib.check(_lib.lib().mico_grads_finite(table.data_ptr(), len(grads), ct.data_ptr(), cs.data_ptr(), n, CHUNK, flag.data_ptr(),
                                                torch.cuda.current_stream(grads[0].device).cuda_stream), "mico_grads_finite")
        return flag

    @torch.no_grad()
    def grad_clip_stats(self, max_grad_norm, grad_mult=1.0, flag=None):
        """The read-only pass of a clipped step over the gradients of all groups: returns the clip coefficient (fp32 device scalar) for
        step(clip_coef=...), records the norm of (gradients * grad_mult) in last_grad_norm and, given `flag`, does grads_nonfinite's job in the
        same launch.  None when no parameter has a gradient.  No host read."""
        max_grad_norm = _check_max_norm(max_grad_norm)
        grads = self._grads()
        if not grads:
            return None
        self.last_grad_norm, coef = _grad_norm_coef(grads, max_grad_norm, grad_mult, flag, self._chunk_cache)
        return coef

    @torch.no_grad()
    def step(self, closure=None, grad_mult=1.0, max_grad_norm=_FROM_ATTRIBUTE, clip_coef=None):
        """grad_mult: gradients are multiplied by it inside the update kernel (GradScaler: 1 / loss scale).
        max_grad_norm (default: the optimizer's attribute; None: no clipping, the launches of an unclipped step exactly): one mico_grad_sumsq over
        all groups' gradients, one mico_grad_clip_coef, then the per-(group, step count) launches read the coefficient from device memory
        (mico_adamw_step_dev).  clip_coef: a coefficient grad_clip_stats already produced for these gradients (GradScaler.step) - used as is."""
        if max_grad_norm is _FROM_ATTRIBUTE:
            max_grad_norm = self.max_grad_norm
        if max_grad_norm is not None:
            _check_max_norm(max_grad_norm)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.lib()
        if clip_coef is None and max_grad_norm is not None:
            clip_coef = self.grad_clip_stats(max_grad_norm, grad_mult)
        refreshed = set()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if not p.is_cuda:
                    raise _lib.MicoHipError("mico_amd.optim.AdamW updates device parameters only (no CPU path)")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p.data, dtype=torch.float32)
                    st["exp_avg_sq"] = torch.zeros_like(p.data, dtype=torch.float32)
                st["step"] += 1
                by_step.setdefault(st["step"], []).append(p)
            for step, plist in by_step.items():
                step_size = group["lr"]
                if group["correct_bias"]:
                    step_size = step_size * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
                dev = plist[0].device
                descs = (_Desc * len(plist))()
                keep = []
                for d, p in zip(descs, plist):
                    st = self.state[p]
                    g = _fp32(p.grad)
                    keep.append(g)
                    assert p.data.is_contiguous() and p.dtype == torch.float32
                    d.p, d.g, d.m, d.v, d.numel = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
                    mir = runtime.weight_mirror(p)
                    if mir is not None:
                        d.w16, d.ld16, d.lo_off, d.cols, d.w16_dtype = mir
                        refreshed.add(runtime.param_uid(p))
                    else:
                        d.w16, d.ld16, d.lo_off, d.cols, d.w16_dtype = None, 0, 0, 1, 0
                table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
                ct, cs, n = self._chunks([p.numel() for p in plist], dev)
                hyper = (float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]), float(step_size),
                         float(grad_mult))
                stream = torch.cuda.current_stream(dev).cuda_stream
                if clip_coef is None:
                    rc = lib.mico_adamw_step(table.data_ptr(), len(plist), ct.data_ptr(), cs.data_ptr(), n, CHUNK, *hyper, stream)
                    _lib.check(rc, "mico_adamw_step")
                else:
                    rc = lib.mico_adamw_step_dev(table.data_ptr(), len(plist), ct.data_ptr(), cs.data_ptr(), n, CHUNK, *hyper,
                                                 clip_coef.data_ptr(), stream)
                    _lib.check(rc, "mico_adamw_step_dev")
                del keep
        runtime.after_optimizer_step(refreshed)
        return loss


class GradScaler:
    """Dynamic loss scaling with the interface and semantics of torch.cuda.amp.GradScaler as the reference trainer uses it
    (data/utils/pipeline.py:30,88,106-107: scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()): the loss is
    multiplied by the scale, step() checks the gradients for inf / NaN and SKIPS the optimizer step when it finds any (one device ->
    host read of a flag, exactly where torch's scaler has its .item()), update() halves the scale after a skipped step and doubles it
    after growth_interval clean ones.  On the MI355X path the un-scaling is not a pass of its own: mico_adamw_step multiplies the
    gradients by 1 / scale while it reads them, and the overflow check is one read-only multi-tensor kernel (mico_grads_finite).
    When the optimizer clips (optimizer.max_grad_norm, or step(optimizer, max_grad_norm=...)), the overflow check and the sum of squares of the
    UN-scaled gradients are one launch (mico_grad_sumsq replaces mico_grads_finite: the same bytes read once), the host read of the flag stays
    the only one, and a skipped step still records optimizer.last_grad_norm (inf / NaN) - the trainer loop above clips unchanged.
    (The engine additionally carries its 16-bit activations' gradients x4096 inside each fp16 function; that internal scale never
    reaches a parameter gradient and is independent of this one.)"""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._scale, self._growth, self._backoff, self._interval = float(init_scale), float(growth_factor), float(backoff_factor), int(growth_interval)
        self._good_steps, self._enabled, self._found_inf = 0, enabled, None

    def scale(self, loss):
        return loss * self._scale if self._enabled else loss

    def get_scale(self):
        return self._scale

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if not hasattr(optimizer, "grads_nonfinite"):
            raise TypeError("mico_amd.optim.GradScaler drives mico_amd.optim.AdamW (fused un-scale + overflow check)")
        dev = next(p for g in optimizer.param_groups for p in g["params"]).device
        max_grad_norm = kwargs["max_grad_norm"] if "max_grad_norm" in kwargs else getattr(optimizer, "max_grad_norm", None)
        if max_grad_norm is not None:
            _check_max_norm(max_grad_norm)
        flag = torch.zeros(1, dtype=torch.float32, device=dev)
        if max_grad_norm is None:
            optimizer.grads_nonfinite(flag)
        else:                                    # the same read of the gradients: overflow flag + norm of the un-scaled gradients -> coefficient
            kwargs["clip_coef"] = optimizer.grad_clip_stats(max_grad_norm, grad_mult=1.0 / self._scale, flag=flag)
        self._found_inf = bool(flag.item())      # the one host sync of the step (torch's GradScaler.step has the same one)
        if self._found_inf:
            return None
        return optimizer.step(*args, grad_mult=1.0 / self._scale, **kwargs)

    def update(self, new_scale=None):
        if not self._enabled:
            return
        if new_scale is not None:
            self._scale, self._good_steps = float(new_scale), 0
        elif self._found_inf is None:
            raise RuntimeError("GradScaler.update() before step(): no inf / nan check was recorded for this iteration")
        elif self._found_inf:
            self._scale, self._good_steps = self._scale * self._backoff, 0
        else:
            self._good_steps += 1
            if self._good_steps == self._interval:
                self._scale, self._good_steps = self._scale * self._growth, 0
        self._found_inf = None

    def state_dict(self):
        return {"scale": self._scale, "growth_factor": self._growth, "backoff_factor": self._backoff, "growth_interval": self._interval,
                "_growth_tracker": self._good_steps} if self._enabled else {}

    def load_state_dict(self, sd):
        if sd:
            self._scale, self._growth, self._backoff = float(sd["scale"]), float(sd["growth_factor"]), float(sd["backoff_factor"])
            self._interval, self._good_steps = int(sd["growth_interval"]), int(sd["_growth_tracker"])


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """Drop-in for torch.nn.utils.clip_grad_norm_(parameters, max_norm) (the commented-out line of data/utils/pipeline.py:102-103), for callers
    that do not step through AdamW(max_grad_norm=...): the gradients are scaled IN PLACE by min(1, max_norm / (total_norm + 1e-6)) and the total
    2-norm comes back as an fp32 device scalar - three launches (mico_grad_sumsq, mico_grad_clip_coef, mico_grads_scale), no host read; gradients
    whose norm is below max_norm keep their bits.  A gradient that is not fp32-contiguous is counted through an fp32 copy and scaled by torch
    (glue, off the hot path).  Only norm_type 2 is provided.  Data parallel: call it after GradBucketReducer.finish() - every rank then holds
    the same averaged gradients and computes the same norm, no collective is needed."""
    if float(norm_type) != 2.0:
        raise ValueError("mico_amd.optim.clip_grad_norm_ provides norm_type=2 only (got {})".format(norm_type))
    max_norm = _check_max_norm(max_norm)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    native = [g for g in grads if g.dtype == torch.float32 and g.is_contiguous()]
    others = [g for g in grads if not (g.dtype == torch.float32 and g.is_contiguous())]
    total_norm, coef = _grad_norm_coef(native + [_fp32(g) for g in others], max_norm)
    if native:
        table, (ct, cs, n) = _grad_table(native)
        _lib.check(_lib.lib().mico_grads_scale(table.data_ptr(), len(native), ct.data_ptr(), cs.data_ptr(), n, CHUNK, coef.data_ptr(),
                                               torch.cuda.current_stream(native[0].device).cuda_stream), "mico_grads_scale")
    for g in others:
        g.mul_(coef.to(g.dtype))
    return total_norm


def build_optimizer(model, args, checkpoint_optim=None):
    """data/utils/build_optimizer.py:11-93.  args.run_cfg: learning_rate, new_lr, clip_lr, weight_decay, betas, optim,
    new_params_name; args.model_cfg.vision_encoder_type.
    Gradient clipping is read from a key of our own, run_cfg.max_grad_norm (absent, None or -1: off) -> optimizer.max_grad_norm.  The
    reference's run_cfg.grad_norm is NOT read: the reference defaults it to 5.0 (data/utils/args.py:230) and then ignores it (the call in
    data/utils/pipeline.py:102-103 is commented out), so honouring it would silently change every existing run."""
    vision_clip = "vision_encoder_type" in args.model_cfg and "clip" in args.model_cfg.vision_encoder_type
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    buckets = {k: [] for k in ("basic", "basic_nd", "new", "new_nd", "clip", "clip_nd")}
    names = {k: [] for k in ("basic", "new", "clip")}
    for k, v in model.named_parameters():
        nd = any(n in k for n in no_decay)
        if any(n in k for n in args.run_cfg.new_params_name):
            kind = "new"
        elif vision_clip and "visual" in k:
            kind = "clip"
        else:
            kind = "basic"
        buckets[kind + ("_nd" if nd else "")].append(v)
        names[kind].append(k)
    rc = args.run_cfg
    groups = [
        {"params": buckets["basic"], "weight_decay": rc.weight_decay, "lr": rc.learning_rate},
        {"params": buckets["basic_nd"], "weight_decay": 0.0, "lr": rc.learning_rate},
        {"params": buckets["new"], "weight_decay": rc.weight_decay, "lr": rc.new_lr},
        {"params": buckets["new_nd"], "weight_decay": 0.0, "lr": rc.new_lr},
        {"params": buckets["clip"], "weight_decay": rc.weight_decay, "lr": rc.clip_lr},
        {"params": buckets["clip_nd"], "weight_decay": 0.0, "lr": rc.clip_lr},
    ]
    if rc.optim != "adamw":
        raise ValueError("invalid optimizer" if rc.optim not in ("adam", "adamax") else
                         f"optimizer '{rc.optim}' is not provided by mico_amd (the MiCo/VAST configs use adamw)")
    for g in groups:
        g["init_lr"] = g["lr"]
    max_grad_norm = getattr(rc, "max_grad_norm", None)
    optimizer = AdamW(groups, lr=rc.learning_rate, betas=rc.betas, max_grad_norm=None if max_grad_norm in (None, -1) else max_grad_norm)
    optimizer.new_params_name = names["new"]
    optimizer.new_lr = rc.new_lr
    optimizer.basic_lr = rc.learning_rate
    optimizer.clip_lr_visual = rc.clip_lr
    optimizer.clip_lr_visual_len = len(buckets["clip"])
    optimizer.zero_grad()
    if checkpoint_optim:
        optimizer.load_state_dict(checkpoint_optim)
    return optimizer
