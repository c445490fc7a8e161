"""Shared by the sliding-window GPU tests: the recording predictor wrapper and a predictor whose output differs
from call to call."""
import torch


class Recorder:
    """Wraps a predictor; keeps a CPU copy of every window batch it was given and every output it returned, and
    the device addresses of both."""

    def __init__(self, fn):
        self.fn, self.inputs, self.outputs = fn, [], []
        self.input_ptrs, self.output_ptrs = [], []

    def __call__(self, x):
        self.inputs.append(x.detach().cpu().clone())
        self.input_ptrs.append(x.data_ptr())
        y = self.fn(x)
        self.outputs.append(y.detach().cpu().clone())
        self.output_ptrs.append(y.data_ptr())
        return y

    def replay(self):
        it = iter(self.outputs)
        return lambda x: next(it)


def noisy(cout, seed):
    """A predictor whose outputs depend on the window content and differ from call to call."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def fn(x):
        base = torch.tanh(x.sum(1, keepdim=True) * 1.7 + 0.3)
        return (base.repeat(1, cout, *([1] * (x.dim() - 2)))
                + 0.1 * torch.randn((x.shape[0], cout) + tuple(x.shape[2:]), device=x.device, generator=g))
    return fn


def at_offset(t, off):
    """A contiguous device copy of `t` that starts `off` elements into its own allocation (off = 1: data_ptr() % 16
    == 4, the alignment no fresh torch allocation has)."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    view = buf[off:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * off) % 16
    return view
