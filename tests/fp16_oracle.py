"""The fp16-operand forward restated on the CPU oracle: ``refcpu._q`` (the rounding of every operand the HIP kernels round) is
replaced, for the duration of a ``with fp16_rounding():`` block, by a rounding through torch.float16 -- round to nearest even,
subnormals kept, overflow to inf, what v_cvt_f16_f32 does.  Straight-through for autograd: the forward alone is emulated.  The same
replacement as tools/fp16_sensitivity.py's forward; nothing under oracle/ is edited."""
import contextlib

import torch

from oracle import refcpu


def _q_fp16(x, emulate_bf16, site=None):
    if not emulate_bf16 or (site is not None and site in refcpu.EXACT_SITES):
        return x
    return x + (x.detach().to(torch.float16).to(x.dtype) - x.detach())


@contextlib.contextmanager
def fp16_rounding():
    """Inside the block, ``emulate_bf16=True`` evaluations of the oracle round their operands to fp16 instead of bf16."""
    orig = refcpu._q
    refcpu._q = _q_fp16
    try:
        yield
    finally:
        refcpu._q = orig
