"""The conv blocks of RoMa-v2's refiners served by this package's HIP kernel.

Each of the model's three ``ConvRefiner`` modules runs its input through nine identical blocks - depthwise 5x5 convolution, eval-mode
BatchNorm, ReLU, 1x1 convolution, under bf16 autocast - as up to four kernels that each read and write the whole activation.
``FusedRefinerBlocks`` finds those blocks under ``model.refiners`` by their structure and, while ``installed(model)`` is active, gives each one
an instance-level ``forward`` backed by ``lfd_refiner_block`` (device tensors) or ``lfd_refiner_block_host`` (CPU tensors): one launch for the
width-32 refiner, the fused depthwise part followed by the block's own ``conv_pointwise`` for any other width.
``core.matcher.RomaMatcher(fused_refiner_blocks=True)`` installs it while a match runs; the model's files are not touched.

The fused block rounds less often than autocast's sequence (which rounds the weights and the depthwise output to bf16 as well), so its results
agree with the model's own within the bound of DESIGN.md 4.18, not bit for bit.  Nothing is approximated silently: what the kernel does not
implement raises ``NotImplementedError``.
"""
from __future__ import annotations

import contextlib
import functools
from typing import Dict, Iterable, List, Tuple

import torch
from torch import nn

from . import hip_backend as hb

_PARTS = ("conv_depthwise", "norm", "relu", "conv_pointwise", "enable_amp")
POINTWISE_WIDTH = 32           # LFD_BLOCK_PW_C: the width whose 1x1 convolution is fused as well
# Hidden widths the shim leaves with torch: by the rule of DESIGN.md 4.18 a width class of the model (32, 128, 512) is taken only if the
# recorded fused call is faster than torch's block at every preset shape of that class.
WIDTHS_LEFT_TO_TORCH: Tuple[int, ...] = ()


def is_block(module: nn.Module) -> bool:
    """The structure ``FusedRefinerBlocks`` recognises: the four sub-modules and the flag of the model's block."""
    return all(hasattr(module, name) for name in _PARTS)


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def check_structure(block: nn.Module) -> int:
    """The block's channel count; NotImplementedError, naming what was found, for anything the kernel does not implement."""
    dw, norm, pw = block.conv_depthwise, block.norm, block.conv_pointwise
    if not isinstance(dw, nn.Conv2d):
        raise NotImplementedError(f"fused refiner block implements a Conv2d depthwise convolution, found {type(dw).__name__}")
    C = int(dw.in_channels)
    if _pair(dw.kernel_size) != (5, 5):
        raise NotImplementedError(f"fused refiner block implements a 5x5 depthwise kernel only, found kernel_size {tuple(dw.kernel_size)}")
    if _pair(dw.stride) != (1, 1) or _pair(dw.dilation) != (1, 1):
        raise NotImplementedError(f"fused refiner block implements stride 1 and dilation 1 only, found stride {tuple(dw.stride)}, "
                                  f"dilation {tuple(dw.dilation)}")
    if isinstance(dw.padding, str) or _pair(dw.padding) != (2, 2) or dw.padding_mode != "zeros":
        raise NotImplementedError(f"fused refiner block implements zero padding of 2 only, found padding {dw.padding!r}, "
                                  f"padding_mode {dw.padding_mode!r}")
    if int(dw.groups) != C or int(dw.out_channels) != C:
        raise NotImplementedError(f"fused refiner block implements a depthwise convolution (groups = in = out channels) only, found "
                                  f"in {dw.in_channels}, out {dw.out_channels}, groups {dw.groups}")
    if not isinstance(norm, nn.BatchNorm2d):
        raise NotImplementedError(f"fused refiner block implements a BatchNorm2d norm only, found {type(norm).__name__}")
    if norm.running_mean is None or norm.running_var is None or norm.weight is None or norm.bias is None or int(norm.num_features) != C:
        raise NotImplementedError("fused refiner block implements a BatchNorm2d with running statistics and affine parameters over the block's "
                                  f"channels only, found track_running_stats {norm.track_running_stats}, affine {norm.affine}, "
                                  f"num_features {norm.num_features}")
    if not isinstance(block.relu, nn.ReLU):
        raise NotImplementedError(f"fused refiner block implements a ReLU activation only, found {type(block.relu).__name__}")
    if (not isinstance(pw, nn.Conv2d) or _pair(pw.kernel_size) != (1, 1) or _pair(pw.stride) != (1, 1) or isinstance(pw.padding, str)
            or _pair(pw.padding) != (0, 0) or int(pw.groups) != 1 or int(pw.in_channels) != C or int(pw.out_channels) != C):
        raise NotImplementedError(f"fused refiner block implements a 1x1 pointwise convolution from {C} to {C} channels only, found {pw!r}")
    return C


class FusedRefinerBlocks:
    """One context per device, made on first use and closed by ``close()``.  Before a device call the context is pointed at torch's current
    stream of that device, so the launch is ordered with the model's own kernels and nothing is synchronised.  The folded parameters of a
    block (s, t, the depthwise weights as (C, 25), the transposed pointwise weights) are computed once, in f64 from the f32 parameters, and
    kept against the parameters' ``data_ptr`` and ``_version``: a parameter modified in place or replaced is folded again."""

    def __init__(self, host_threads: int = 0, skip_widths: Iterable[int] = WIDTHS_LEFT_TO_TORCH):
        self._host_threads = int(host_threads)
        self._skip = frozenset(int(w) for w in skip_widths)
        self._ctx: Dict[torch.device, object] = {}
        self._folded: Dict[int, Tuple[tuple, tuple]] = {}

    def _context(self, device: torch.device):
        ctx = self._ctx.get(device)
        if ctx is None:
            ctx = hb.HostDensifier(self._host_threads) if device.type == "cpu" else hb.HipDensifier(device)
            self._ctx[device] = ctx
        return ctx

    def blocks(self, model: nn.Module) -> List[nn.Module]:
        """The blocks under ``model.refiners`` this object serves, in module order; a block of unsupported structure raises."""
        found = [m for m in model.refiners.modules() if is_block(m)]
        return [m for m in found if check_structure(m) not in self._skip]

    def _fold(self, block: nn.Module, C: int, device: torch.device):
        dw, norm, pw = block.conv_depthwise, block.norm, block.conv_pointwise
        sources = [dw.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var, pw.weight] + [b for b in (dw.bias, pw.bias) if b is not None]
        key = tuple((int(t.data_ptr()), int(t._version), str(t.device)) for t in sources) + (float(norm.eps), str(device))
        kept = self._folded.get(id(block))
        if kept is not None and kept[0] == key:
            return kept[1]
        for t in sources:
            if t.dtype != torch.float32:
                raise NotImplementedError(f"fused refiner block folds float32 parameters only, found {t.dtype}")
        with torch.no_grad():
            s = norm.weight.double() / torch.sqrt(norm.running_var.double() + float(norm.eps))
            b_dw = dw.bias.double() if dw.bias is not None else torch.zeros(C, dtype=torch.float64, device=s.device)
            t = norm.bias.double() + (b_dw - norm.running_mean.double()) * s
            folded = [dw.weight.detach().reshape(C, 25).contiguous(), s.float(), t.float()]
            if C == POINTWISE_WIDTH:
                pb = pw.bias.detach() if pw.bias is not None else torch.zeros(C, dtype=torch.float32, device=s.device)
                folded += [pw.weight.detach().reshape(C, C).t().contiguous(), pb.contiguous()]
            folded = tuple(f.to(device) for f in folded)
        self._folded[id(block)] = (key, folded)
        return folded

    def forward(self, block: nn.Module, x: torch.Tensor) -> torch.Tensor:
        """The block's forward: what ``installed`` puts in the place of the module's own."""
        C = check_structure(block)
        if block.training:
            raise NotImplementedError("fused refiner block implements eval mode only (running statistics), the block is in training mode")
        if not block.enable_amp:
            raise NotImplementedError("fused refiner block implements the bf16 autocast path only, the block has enable_amp False")
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"fused refiner block implements float32 and bfloat16 input only, got {getattr(x, 'dtype', type(x).__name__)}")
        if x.requires_grad:
            raise NotImplementedError("fused refiner block has no backward pass, the input requires grad")
        if x.dim() != 4 or int(x.shape[1]) != C:
            raise NotImplementedError(f"fused refiner block implements (B, {C}, H, W) input only, got {tuple(x.shape)}")
        device = x.device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        ctx = self._context(device)
        if device.type != "cpu":
            ctx.set_stream(torch.cuda.current_stream(device))
        folded = self._fold(block, C, device)
        if C == POINTWISE_WIDTH:
            return ctx.refiner_block(x, *folded)
        hidden = ctx.refiner_block(x, *folded)
        with torch.autocast(device_type=device.type, enabled=True, dtype=torch.bfloat16):
            return block.conv_pointwise(hidden)

    @contextlib.contextmanager
    def installed(self, model: nn.Module):
        """While the body runs, every block under ``model.refiners`` has this object's fused forward as an instance attribute; what was there
        before - usually nothing, the class's method - comes back afterwards, also when the body raises."""
        previous = []
        try:
            for block in self.blocks(model):
                previous.append((block, "forward" in block.__dict__, block.__dict__.get("forward")))
                block.forward = functools.partial(self.forward, block)
            yield
        finally:
            for block, had, value in reversed(previous):
                if had:
                    block.__dict__["forward"] = value
                else:
                    block.__dict__.pop("forward", None)

    def close(self) -> None:
        for ctx in self._ctx.values():
            ctx.close()
        self._ctx.clear()
        self._folded.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
