"""The fp16-operand BACKWARD restated on the CPU oracle (tools/fp16_sensitivity.py's emulation, as a context manager for the tests):
inside ``with fp16_grad_rounding(s):`` the oracle's rounding function ``refcpu._q`` rounds every forward operand through torch.float16
(straight-through) and, at every activation site (not the ".w" weight sites, whose gradients the kernels form in f32), rounds the
gradient flowing back through it as the kernels store it: g -> fp16(g * 2^s) / 2^s.  Nothing under oracle/ is edited."""
import contextlib

import torch

from oracle import refcpu


class _GradRound(torch.autograd.Function):
    """Identity forward; the backward rounds the scaled gradient to fp16 and removes the scale (exact: a power of two)."""

    @staticmethod
    def forward(ctx, x, log2_scale):
        ctx.scale = 2.0 ** log2_scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (g * ctx.scale).to(torch.float16).to(g.dtype) / ctx.scale, None


@contextlib.contextmanager
def fp16_grad_rounding(log2_scale):
    """Inside the block, ``emulate_bf16=True`` evaluations of the oracle round operands to fp16 and their gradients to scaled fp16."""
    orig = refcpu._q

    def q(x, emulate_bf16, site=None):
        if not emulate_bf16 or (site is not None and site in refcpu.EXACT_SITES):
            return x
        y = x + (x.detach().to(torch.float16).to(x.dtype) - x.detach())
        if x.requires_grad and not (site or "").endswith(".w"):
            y = _GradRound.apply(y, log2_scale)
        return y

    refcpu._q = q
    try:
        yield
    finally:
        refcpu._q = orig
