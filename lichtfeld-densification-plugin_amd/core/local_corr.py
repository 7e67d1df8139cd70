"""RoMa-v2's local correlation served by this package's HIP kernel.

``romav2.local_correlation`` does ``import local_corr`` - a CUDA-only extension - and calls ``local_corr.local_corr(feature0, feature1, warp,
mode=..., normalized_coords=...)`` when the import worked; without it the model materialises the sampled neighbour features as a (C, h, w, K)
tensor.  ``LocalCorr`` is an object with that call, backed by ``lfd_local_corr`` (device tensors) or ``lfd_local_corr_host`` (CPU tensors).
``core.matcher.RomaMatcher(fused_local_corr=True)`` puts it in the extension's place while a match runs; the model's files are not touched.

Nothing is approximated silently: what the kernel does not implement raises ``NotImplementedError``.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import hip_backend as hb


class LocalCorr:
    """``local_corr(feature0 (B, N, C), feature1 (B, H1, W1, C), warp (B, N, K, 2)) -> (B, N, K)``, f32, forward only.

    One context per device, made on first use and closed by ``close()``.  Before a device call the context is pointed at torch's current
    stream of that device, so the launch is ordered with the model's own kernels and nothing is synchronised (changing the stream waits for
    what this object issued on the previous one: lfd_set_stream)."""

    def __init__(self, host_threads: int = 0):
        self._host_threads = int(host_threads)
        self._ctx: Dict[torch.device, object] = {}

    def _context(self, device: torch.device):
        ctx = self._ctx.get(device)
        if ctx is None:
            ctx = hb.HostDensifier(self._host_threads) if device.type == "cpu" else hb.HipDensifier(device)
            self._ctx[device] = ctx
        return ctx

    def local_corr(self, feature0: torch.Tensor, feature1: torch.Tensor, warp: torch.Tensor, mode: str = "bilinear",
                   normalized_coords: bool = True) -> torch.Tensor:
        if mode != "bilinear":
            raise NotImplementedError(f"fused local_corr implements mode='bilinear' only, got {mode!r}")
        if not normalized_coords:
            raise NotImplementedError("fused local_corr implements normalized_coords=True only")
        for name, t in (("feature0", feature0), ("feature1", feature1), ("warp", warp)):
            if t.dtype != torch.float32:
                raise NotImplementedError(f"fused local_corr implements float32 only, {name} is {t.dtype}")
            if t.requires_grad:
                raise NotImplementedError(f"fused local_corr has no backward pass, {name} requires grad")
        device = feature0.device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        ctx = self._context(device)
        if device.type != "cpu":
            ctx.set_stream(torch.cuda.current_stream(device))
        return ctx.local_corr(feature0, feature1, warp)

    __call__ = local_corr

    def close(self) -> None:
        for ctx in self._ctx.values():
            ctx.close()
        self._ctx.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
