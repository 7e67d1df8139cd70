"""The output head of RoMa-v2's refiners served by this package's HIP kernel.

Behind its nine conv blocks each of the model's three ``ConvRefiner`` modules casts the activation to f32, runs two 1x1 convolutions
(hidden -> 2, hidden -> 4) and about a dozen element-wise kernels on 2- and 4-channel tensors: the warp update, softplus, the
Cholesky-to-precision conversion and the addition of the previous state.  That tail is written inline in the refiner's ``forward``, so the
only seam is the ``forward`` itself: ``FusedRefinerHead`` finds the refiners under ``model.refiners`` by their structure and, while
``installed(model)`` is active, gives each one an instance-level ``forward`` that runs the refiner's own sub-modules up to ``z`` and then ONE
``lfd_refiner_head`` (device tensors) or ``lfd_refiner_head_host`` (CPU tensors) call.
``core.matcher.RomaMatcher(fused_refiner_head=True)`` installs it while a match runs; the model's files are not touched.

The front half calls ``proj``, ``disp_emb``, ``block1`` and ``hidden_blocks`` of the refiner and looks ``bhwc_grid_sample``,
``get_normalized_grid`` and ``local_correlation`` up, at every call, in the module that defines the refiner's class - so the fused local
correlation and the fused conv blocks keep working beneath it.  The fused tail agrees with the model's own f32 tail within the bound of
DESIGN.md 4.20, not bit for bit.  Nothing is approximated silently: what the kernel does not implement raises ``NotImplementedError``.
"""
from __future__ import annotations

import contextlib
import functools
import sys
from typing import Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn

from . import hip_backend as hb

_PARTS = ("proj", "disp_emb", "block1", "hidden_blocks", "warp_head", "confidence_head", "cfg")
_FUNCTIONS = ("bhwc_grid_sample", "get_normalized_grid", "local_correlation")
# Hidden widths the shim leaves with torch: by the rule of DESIGN.md 4.20 (4.18's) a width class of the model (32, 128, 512) is taken only if
# the recorded fused call is faster than torch's tail at every preset shape of that class (profiles/r22/refiner_head.txt).
WIDTHS_LEFT_TO_TORCH: Tuple[int, ...] = ()


def is_refiner(module: nn.Module) -> bool:
    """The structure ``FusedRefinerHead`` recognises: the sub-modules and the configuration of the model's conv refiner."""
    return all(hasattr(module, name) for name in _PARTS)


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _is_1x1(conv) -> bool:
    return (isinstance(conv, nn.Conv2d) and _pair(conv.kernel_size) == (1, 1) and _pair(conv.stride) == (1, 1) and not isinstance(conv.padding, str)
            and _pair(conv.padding) == (0, 0) and _pair(conv.dilation) == (1, 1) and int(conv.groups) == 1)


def check_structure(refiner: nn.Module) -> int:
    """The refiner's hidden width; NotImplementedError, naming what was found, for anything the kernel does not implement."""
    wh, ch, cfg = refiner.warp_head, refiner.confidence_head, refiner.cfg
    if not _is_1x1(wh) or int(wh.out_channels) != 2:
        raise NotImplementedError(f"fused refiner head implements a 1x1 Conv2d warp head (stride 1, no padding, groups 1) to 2 channels only, found {wh!r}")
    C = int(wh.in_channels)
    if not _is_1x1(ch) or int(ch.out_channels) != 4 or int(ch.in_channels) != C:
        raise NotImplementedError(f"fused refiner head implements a 1x1 Conv2d confidence head (stride 1, no padding, groups 1) from {C} to 4 "
                                  f"channels only, found {ch!r}")
    for t in [wh.weight, ch.weight] + [b for b in (wh.bias, ch.bias) if b is not None]:
        if t.dtype != torch.float32:
            raise NotImplementedError(f"fused refiner head implements float32 head parameters only, found {t.dtype}")
    if int(getattr(cfg, "warp_dim", -1)) != 2 or int(getattr(cfg, "confidence_dim", -1)) != 4:
        raise NotImplementedError(f"fused refiner head implements warp_dim 2 and confidence_dim 4 only, found warp_dim {getattr(cfg, 'warp_dim', None)}, "
                                  f"confidence_dim {getattr(cfg, 'confidence_dim', None)}")
    if getattr(cfg, "grid_sample_mode", None) != "bilinear":
        raise NotImplementedError(f"fused refiner head implements grid_sample_mode 'bilinear' only, found {getattr(cfg, 'grid_sample_mode', None)!r}")
    if bool(getattr(cfg, "channels_last", False)):
        raise NotImplementedError("fused refiner head implements contiguous NCHW activations only, found channels_last True")
    return C


class FusedRefinerHead:
    """One context per device, made on first use and closed by ``close()``.  Before a device call the context is pointed at torch's current
    stream of that device, so the launch is ordered with the model's own kernels and nothing is synchronised.  The concatenated head weights
    (6, C) and bias (6) of a refiner are built once per device and kept against the parameters' ``data_ptr`` and ``_version``: a parameter
    modified in place or replaced is concatenated again."""

    def __init__(self, host_threads: int = 0, skip_widths: Iterable[int] = WIDTHS_LEFT_TO_TORCH):
        self._host_threads = int(host_threads)
        self._skip = frozenset(int(w) for w in skip_widths)
        self._ctx: Dict[torch.device, object] = {}
        self._heads: Dict[Tuple[int, str], Tuple[tuple, tuple]] = {}

    def _context(self, device: torch.device):
        ctx = self._ctx.get(device)
        if ctx is None:
            ctx = hb.HostDensifier(self._host_threads) if device.type == "cpu" else hb.HipDensifier(device)
            self._ctx[device] = ctx
        return ctx

    def refiners(self, model: nn.Module) -> List[nn.Module]:
        """The refiners under ``model.refiners`` this object serves, in module order; a refiner of unsupported structure raises."""
        found = [m for m in model.refiners.modules() if is_refiner(m)]
        return [m for m in found if check_structure(m) not in self._skip]

    def _head(self, refiner: nn.Module, C: int, device: torch.device):
        wh, ch = refiner.warp_head, refiner.confidence_head
        sources = [wh.weight, ch.weight] + [b for b in (wh.bias, ch.bias) if b is not None]
        key = tuple((int(t.data_ptr()), int(t._version), str(t.device)) for t in sources) + (wh.bias is None, ch.bias is None)
        kept = self._heads.get((id(refiner), str(device)))
        if kept is not None and kept[0] == key:
            return kept[1]
        with torch.no_grad():
            bias = [m.bias.detach() if m.bias is not None else torch.zeros(n, dtype=torch.float32, device=m.weight.device) for m, n in ((wh, 2), (ch, 4))]
            head = (torch.cat([wh.weight.detach().reshape(2, C), ch.weight.detach().reshape(4, C)], 0).to(device).contiguous(),
                    torch.cat(bias, 0).to(device).contiguous())
        self._heads[(id(refiner), str(device))] = (key, head)
        return head

    def front(self, refiner: nn.Module, f_A: torch.Tensor, f_B: torch.Tensor, prev_warp: torch.Tensor, scale_factor: torch.Tensor) -> torch.Tensor:
        """``z``: the activation behind the refiner's nine blocks, computed by its own sub-modules from the projected features of A, those of B
        sampled at ``prev_warp``, the embedded displacement and - where the refiner has one - the local correlation."""
        cfg = refiner.cfg
        ns = sys.modules[type(refiner).__module__]
        sample, grid_of, correlate = (getattr(ns, name) for name in _FUNCTIONS)
        B, H, W, D = (int(v) for v in f_A.shape)
        if tuple(f_B.shape) != (B, H, W, D) or D != int(cfg.feat_dim):
            raise ValueError(f"fused refiner head: f_A {tuple(f_A.shape)} and f_B {tuple(f_B.shape)} must both be (B, H, W, {cfg.feat_dim})")
        project = lambda f: refiner.proj(f.reshape(B, H * W, D).float()).reshape(B, H, W, int(cfg.proj_dim))     # noqa: E731
        feat_a, feat_b = project(f_A), project(f_B)
        with torch.no_grad():
            feat_b_at_a = sample(feat_b, prev_warp, mode=cfg.grid_sample_mode, align_corners=False)
        displacement = (prev_warp - grid_of(B, H, W)).permute(0, 3, 1, 2)
        embedded = refiner.disp_emb(scale_factor[None, :, None, None] * displacement)
        a_chw, b_chw = feat_a.permute(0, 3, 1, 2), feat_b_at_a.permute(0, 3, 1, 2)
        d = torch.cat((a_chw, b_chw, embedded), dim=1)
        if cfg.local_corr_radius is not None:
            corr = correlate(a_chw, b_chw, local_radius=cfg.local_corr_radius, warp=prev_warp, scale_factor=scale_factor)
            d = torch.cat((d, corr), dim=1)
        return refiner.hidden_blocks(refiner.block1(d))

    def forward(self, refiner: nn.Module, *, f_A: torch.Tensor, f_B: torch.Tensor, prev_warp: torch.Tensor,
                prev_confidence: Optional[torch.Tensor], scale_factor: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The refiner's forward: what ``installed`` puts in the place of the module's own."""
        C = check_structure(refiner)
        if refiner.training:
            raise NotImplementedError("fused refiner head implements eval mode only, the refiner is in training mode")
        for name, t in (("f_A", f_A), ("f_B", f_B), ("prev_warp", prev_warp), ("prev_confidence", prev_confidence), ("scale_factor", scale_factor)):
            if t is not None and t.requires_grad:
                raise NotImplementedError(f"fused refiner head has no backward pass, {name} requires grad")
        device = f_A.device
        if torch.is_autocast_enabled(device.type):
            raise NotImplementedError("fused refiner head implements the model's float32 heads only, autocast is enabled around the refiner")
        if prev_confidence is not None and int(prev_confidence.shape[-1]) not in (1, 4):
            raise NotImplementedError(f"fused refiner head implements a previous confidence of 1 or 4 channels only, got {int(prev_confidence.shape[-1])}")
        for name, t in (("prev_warp", prev_warp), ("prev_confidence", prev_confidence)):
            if t is not None and t.dtype != torch.float32:
                raise NotImplementedError(f"fused refiner head implements a float32 {name} only, got {t.dtype}")
        prev_warp = prev_warp.detach()
        if prev_confidence is not None:
            prev_confidence = prev_confidence.detach()
        return self.tail(refiner, self.front(refiner, f_A, f_B, prev_warp, scale_factor), prev_warp, prev_confidence, C)

    def tail(self, refiner: nn.Module, z: torch.Tensor, prev_warp: torch.Tensor, prev_confidence: Optional[torch.Tensor],
             C: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Everything behind the ninth block: one ``refiner_head`` call on torch's current stream."""
        C = check_structure(refiner) if C is None else C
        if z.dtype not in (torch.bfloat16, torch.float32):
            raise NotImplementedError(f"fused refiner head implements a bfloat16 or float32 activation only, the blocks returned {z.dtype}")
        if z.dim() != 4 or int(z.shape[1]) != C:
            raise NotImplementedError(f"fused refiner head implements a (B, {C}, H, W) activation only, the blocks returned {tuple(z.shape)}")
        if not z.is_contiguous():
            raise NotImplementedError(f"fused refiner head implements a contiguous NCHW activation only, the blocks returned strides {tuple(z.stride())} "
                                      f"for shape {tuple(z.shape)}")
        if z.requires_grad:
            raise NotImplementedError("fused refiner head has no backward pass, the activation requires grad (run the model under no_grad)")
        device = z.device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        ctx = self._context(device)
        if device.type != "cpu":
            ctx.set_stream(torch.cuda.current_stream(device))
        head_w, head_b = self._head(refiner, C, device)
        warp, confidence = ctx.refiner_head(z, head_w, head_b, prev_warp, prev_confidence, float(refiner.cfg.refine_init))
        return {"warp": warp, "confidence": confidence}

    @contextlib.contextmanager
    def installed(self, model: nn.Module):
        """While the body runs, every refiner under ``model.refiners`` has this object's forward as an instance attribute; what was there
        before - usually nothing, the class's method - comes back afterwards, also when the body raises."""
        previous = []
        try:
            for refiner in self.refiners(model):
                previous.append((refiner, "forward" in refiner.__dict__, refiner.__dict__.get("forward")))
                refiner.forward = functools.partial(self.forward, refiner)
            yield
        finally:
            for refiner, had, value in reversed(previous):
                if had:
                    refiner.__dict__["forward"] = value
                else:
                    refiner.__dict__.pop("forward", None)

    def close(self) -> None:
        for ctx in self._ctx.values():
            ctx.close()
        self._ctx.clear()
        self._heads.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
