"""One fused training step on the caller's thread: forward, weighted CE, backward (+ optimizer), and
`TrainStepper`, the per-batch step of `model_utils.train` (replayed as one hipGraph per batch shape).

`loss = crit(model(hsi, lidar), target); loss.backward(); opt.step()` is the reference loop
(model_utils.py:918-934) and works unchanged with this package.  Its backward, however, runs on
the autograd engine's device thread, from which the step's side streams cannot be forked inside
a hipGraph capture on this ROCm release.  `fused_train_step` issues the SAME kernels (same
program, same numerics: tests/test_model_gpu.py checks both entry points agree bit-for-bit)
from the caller's thread, so a training loop or the benchmark can capture the whole
multi-stream step — forward, CE, backward and AdamW — into one hipGraph.
"""
from __future__ import annotations

import inspect
from functools import partial

import torch

from . import parallel, seeds
from .flat import FlatParams, expose_grad_views
from .losses import Cross_fusion_CNN_Loss, CrossEntropyLoss, EndNet_Loss, GLT_Loss, ce_forward_backward
from .model import Multimodality_Mamba, _Program
from .optim import AdamW
from .program import counters


def fused_train_step(model: Multimodality_Mamba, criterion: CrossEntropyLoss, hsi, lidar, target,
                     optimizer=None, grad_hook=None, exchange=None):
    """Returns the loss tensor (device scalar).  Gradients land in `model.flat_params.grad`
    (accumulated like autograd if a gradient is already present); `grad_hook(model)` runs between
    backward and the optimizer step.  `exchange` (parallel.GradExchange) all-reduces the gradient
    bucket by bucket on its own stream while the backward is still running, and the optimizer step
    is ordered after the last bucket."""
    if not model.training:
        raise RuntimeError("fused_train_step needs the model in train mode")
    if hsi.device.type != "cuda":
        raise RuntimeError("ViT-CNN MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
    model._ensure_flat()
    hsi = hsi.detach().to(torch.float32).contiguous()
    lidar = lidar.detach().to(torch.float32).contiguous()
    target = target.to(torch.int64).contiguous()
    prog = _Program(model, hsi.device, hsi.shape[0], True, "grad")
    logits = prog.forward(hsi, lidar)
    w = criterion.weight
    if w is not None and w.device != logits.device:
        w = w.to(logits.device)
    loss, dlog = ce_forward_backward(logits, target, w, criterion.ignore_index)
    flat = model.flat_params
    if exchange is not None:
        if flat.grad is not None:
            raise RuntimeError("fused_train_step(exchange=...): zero the gradients first (set_to_none)")
        grad = exchange.begin(model, hsi.device)
        prog.backward(dlog, bucket_hook=exchange.bucket_ready, out=grad)
        exchange.finish(optimizer)
        flat.grad = grad
    else:
        grad = prog.backward(dlog)
        if flat.grad is None:
            flat.grad = grad
        else:
            flat.grad.add_(grad)
    expose_grad_views(model)
    if grad_hook is not None:
        grad_hook(model)
    if optimizer is not None:
        optimizer.step()
    return loss


class _Captured:
    """One batch shape's captured step: static inputs, the graph, and its loss / gradient outputs."""

    def __init__(self, hsi, lidar, target):
        self.hsi, self.lidar, self.target = hsi, lidar, target
        self.graph = torch.cuda.CUDAGraph()
        self.loss = None
        self.grad = None


def _capture_step_blocker(net, optimizer, criterion):
    """why `capture_step=True` cannot capture this model / optimizer / criterion (None: it can)"""
    if not isinstance(net, FlatParams) or isinstance(net, Multimodality_Mamba):
        return "not one of the package's comparison models"
    try:
        params = [p for p in inspect.signature(net.forward).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) and p.default is p.empty]
    except (TypeError, ValueError):
        params = []
    if len(params) != 2:
        return "the model's forward does not take two inputs"
    if not isinstance(optimizer, AdamW) or optimizer._owner() is not net:
        return "the optimizer is not the package's fused AdamW / Adam over this model"
    if not isinstance(criterion, (CrossEntropyLoss, Cross_fusion_CNN_Loss, EndNet_Loss, GLT_Loss)):
        return "the criterion is not one of the package's losses"
    return None


class TrainStepper:
    """The optimizer step `model_utils.train` runs per batch (model_utils.py:918-934: zero_grad,
    forward, criterion, backward, step), as fast as the model allows:

    * ViT-CNN with the fused AdamW: the whole step — forward, CE, backward, (data parallel: the three
      head-first gradient buckets all-reduced by RCCL on a side stream while the backward runs,
      parallel.GradExchange), AdamW — is `fused_train_step`, captured once per batch shape into a
      hipGraph and replayed for every later batch of that shape.  The first batch of a shape runs the
      same step eagerly (it is a real update, and it builds the persistent workspaces the capture
      records); the second is captured and replayed; capture does not run the step, so every batch is
      exactly one update.  A short last batch is simply another shape.  The optimizer's
      hyper-parameters live in device memory and are synced before each replay (`AdamW.sync_hyper`),
      so StepLR's lr changes take effect as with torch.optim.
    * anything else (torch modules / optimizers, `s2eft.ViT`'s one-input forward over token rows, FusAtNet):
      the reference's eager sequence, with `parallel.allreduce_gradients` between backward and step under DP.
    * `capture_step=True` (opt-in): the comparison models -- a flat-parameter model other
      than ViT-CNN with a two-input forward, stepped by the fused AdamW / Adam under one of the package's losses --
      follow the same protocol through autograd: the first batch of a shape runs `zero_grad; crit(net(x1, x2),
      t).backward(); opt.step()` eagerly, the second captures exactly that into a hipGraph, later ones copy into the
      static inputs and replay.  The dropout masks' seed lives in device memory (`seeds.attach`; attached here from
      torch's CPU generator if the model has dropout and none is attached) and `vc_seed_next` is the first launch
      of every step, eager or replayed: step n uses `seeds.step_seed(base, n)` whichever way it ran, and a replay
      draws fresh masks.  Under data parallelism this path is off: the eager sequence above, and `launch` says so.

    `launch` says which path ran ("hipGraph", "eager", or why not / the capture failure), never silently."""

    def __init__(self, net, optimizer, criterion, use_graph: bool = True, capture_step: bool = False):
        self.net, self.opt, self.crit = net, optimizer, criterion
        self.capture_step = bool(capture_step)
        self.fused = (isinstance(net, Multimodality_Mamba) and isinstance(optimizer, AdamW)
                      and isinstance(criterion, CrossEntropyLoss))
        self.use_graph = use_graph and self.fused
        self.graphs = {}
        self.seen = set()
        self.binding = None
        self.launch = "hipGraph" if self.use_graph else "eager"
        self.exchange = None
        if self.fused and parallel.is_distributed():
            self.exchange = parallel.GradExchange(net)
            optimizer.grad_scale = 1.0 / parallel.world()
            if self.use_graph and not parallel.capturable():
                # gloo's host-side collectives cannot be captured: the same fused step, eagerly
                self.use_graph = False
                self.launch = "eager (the gloo exchange is not graph-capturable)"
        # the comparison models' captured step
        self.generic = False
        if self.capture_step and not self.fused:
            why = _capture_step_blocker(net, optimizer, criterion)
            if why is None and parallel.is_distributed():
                why = "data parallel: the gradient all-reduce of this path is not captured"
            if why is not None:
                self.launch = f"eager (capture_step: {why})"
            else:
                self.generic = True
                self.use_graph = bool(use_graph)
                self.launch = "hipGraph" if self.use_graph else "eager"
                self._drops = seeds.has_dropout(net)   # read once: a captured graph bakes every p in anyway

    @property
    def replays(self) -> bool:
        """the returned loss may be a replayed graph's buffer, overwritten by the next step: clone it to keep it"""
        return self.fused or self.generic

    def _check_binding(self):
        """captured graphs hold the parameter / buffer / optimizer-state addresses of their capture:
        drop them if the model was re-flattened (load_state_dict with assign, .to(), ...)"""
        m = self.net
        if self.generic:
            # FlatParams re-packs into a NEW flat buffer on every device move / parameter replacement (buffers move
            # with it: nn.Module._apply), so its address stands for the module's storage; plus the optimizer state
            # and the seed state the launches were recorded with, and the model's precision where it has one (FusAtNet:
            # the recorded conv launches carry it) and its conv mode (MHST: which family the graph launches)
            st = seeds.state(m)
            key = (m._flat_store.data_ptr(), id(self.opt._dev["m"]) if self.opt._dev is not None else None,
                   st.state_ptr if st is not None else None, getattr(m, "precision", None), getattr(m, "conv", None))
            if key != self.binding:
                self.graphs, self.seen = {}, set()
                self.binding = key
            return
        key = (m._bind_gen, m._flat_store.data_ptr(), m._bflat.data_ptr(), m._iflat.data_ptr(),
               id(self.opt._dev["m"]) if self.opt._dev is not None else None)
        if key != self.binding:
            self.graphs, self.seen = {}, set()
            self.binding = key

    def _fused_step(self, data, data2, target):
        return fused_train_step(self.net, self.crit, data, data2, target, optimizer=self.opt, exchange=self.exchange)

    def _autograd_step(self, st, data, data2, target):
        """the reference sequence on the current stream, the seed advanced first; eager and captured alike"""
        if st is not None:
            st.advance()
        loss = self.crit(self.net(data, data2), target)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def _capture(self, key, run, data, data2, target, target_dtype):
        """`run(hsi, lidar, target)` over static copies of this batch's shapes, captured into a hipGraph"""
        dev = data.device
        c = _Captured(torch.empty_like(data, memory_format=torch.contiguous_format),
                      torch.empty_like(data2, memory_format=torch.contiguous_format),
                      torch.empty(target.shape, dtype=target_dtype, device=dev))
        torch.cuda.synchronize(dev)
        self.opt.sync_hyper()          # nothing may change inside the capture (AdamW.step's copy)
        self.opt.zero_grad(set_to_none=True)
        ctx = torch.cuda.graph(c.graph)
        if self.generic:
            # the capture stream's arrival counters (cached per stream for the process) are created and zeroed now,
            # not by a node of this graph: a capture that fails would otherwise leave them cached and never zeroed
            counters(dev, ctx.capture_stream.cuda_stream)
        try:
            with ctx:
                c.loss = run(c.hsi, c.lidar, c.target)
        except RuntimeError as e:    # reported through `launch`, and every shape stays eager
            torch.cuda.synchronize(dev)
            self.opt.zero_grad(set_to_none=True)
            self.launch = f"eager (graph capture failed: {str(e)[:100]})"
            self.use_graph = False
            return None
        c.grad = self.net.flat_params.grad
        self.graphs[key] = c
        return c

    def step(self, data, data2, target):
        """one optimizer step on this batch; returns the loss as a device scalar"""
        net = self.net
        if not (self.fused or self.generic):
            self.opt.zero_grad()
            out = net(data, data2)
            loss = self.crit(out, target)
            loss.backward()
            parallel.allreduce_gradients(net, self.opt)
            self.opt.step()
            return loss
        dev = net.flat_params.device
        data = data.to(dev, non_blocking=True)
        data2 = data2.to(dev, non_blocking=True)
        target = target.to(dev, non_blocking=True)
        net._ensure_flat()
        self.opt._device_state(net.flat_params)   # the optimizer state exists before the binding is taken
        if self.generic:
            st = seeds.state(net)
            if st is None and self._drops:
                st = seeds.attach(net)
            run, target_dtype = partial(self._autograd_step, st), target.dtype
            key = (tuple(data.shape), data.dtype, tuple(data2.shape), data2.dtype, tuple(target.shape), target.dtype)
        else:
            run, target_dtype = self._fused_step, torch.int64
            key = (tuple(data.shape), tuple(data2.shape), tuple(target.shape))
        self._check_binding()
        c = self.graphs.get(key)
        if c is None and self.use_graph and key in self.seen:
            c = self._capture(key, run, data, data2, target, target_dtype)
        self.seen.add(key)
        if c is None:
            self.opt.zero_grad(set_to_none=True)
            return run(data, data2, target)
        c.hsi.copy_(data)
        c.lidar.copy_(data2)
        c.target.copy_(target)
        self.opt.sync_hyper()
        c.graph.replay()
        net.flat_params.grad = c.grad
        return c.loss
