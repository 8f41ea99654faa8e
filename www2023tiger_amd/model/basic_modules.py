"""MergeLayer and MLP (reference: tiger/model/basic_modules.py:5-33).  MLP is the node-classification decoder
(train_supervised.py); on the GPU its forward and backward are the library's fused kernels (tg_decoder_fwd /
tg_decoder_bwd)."""
import ctypes as C

import torch
from torch import Tensor, nn

from .._lib import TgDecoder, check, lib, ptr
from ..hip_ops import stream_ptr
from .dense import hip_autograd, hip_inference, linear_autograd, linear_forward

DECODER_MAX_D = 512  # tiger_hip.h: TG_DECODER_MAX_D


class MergeLayer(nn.Module):
    """Two-layer perceptron on a concatenated pair: fc2(dropout(relu(fc1([x1 | x2])))).
    `fc1` / `fc2` / `dropout` are the reference's attribute names (state_dict keys, dropout
    probability read by the training step).  Inside the HIP path the two layers are consumed
    as raw weights (tg_linear); on the operator path this forward runs the same kernels - under no_grad directly,
    under autograd through an autograd function whose backward is the library's too (tg_linear_bwd)."""

    def __init__(self, dim1: int, dim2: int, hidden_size: int, out_size: int, dropout: float = 0.):
        super().__init__()
        layers = {'fc1': nn.Linear(dim1 + dim2, hidden_size), 'fc2': nn.Linear(hidden_size, out_size)}
        for name, layer in layers.items():
            nn.init.xavier_normal_(layer.weight)  # biases keep nn.Linear's default, as in the reference
            self.add_module(name, layer)
        self.dropout = nn.Dropout(dropout)
        self.act = nn.ReLU()

    def forward(self, x1, x2):
        x = torch.cat((x1, x2), dim=-1)
        if hip_inference(x, self.dropout, self.fc1, self.fc2):  # the library's MFMA kernels (tg_linear_fwd), ReLU fused
            return linear_forward(self.fc2, linear_forward(self.fc1, x, relu=True))
        if hip_autograd(x, self.fc1, self.fc2):  # autograd / active dropout: the same kernels through an autograd function
            return linear_autograd(self.fc2, self.dropout(self.act(linear_autograd(self.fc1, x))))
        return self.fc2(self.dropout(self.act(self.fc1(x))))  # CPU tensors, widths the kernels do not take: plain torch


def _decoder_struct(ts) -> TgDecoder:
    return TgDecoder(*(ptr(t) for t in ts))


def decoder_forward(params, x: Tensor, out: Tensor, p: float = 0.0, key: Tensor = None, z1: Tensor = None,
                    z2: Tensor = None) -> Tensor:
    """tg_decoder_fwd: logits of the rows of x [n, d] into out [n] (any contiguous float32 slice); params = (w1, b1, w2,
    b2, w3, b3); p > 0: dropout with the mask stream of key = device int64 {seed, counter}; z1 / z2: saved
    pre-activations (nullable)."""
    w = _decoder_struct(params)
    check(lib.tg_decoder_fwd(x.shape[0], ptr(x), x.shape[1], C.byref(w), float(p), ptr(key) if p > 0 else None, ptr(out),
                             ptr(z1), ptr(z2), stream_ptr(x.device)), 'tg_decoder_fwd')
    return out


class _DecoderFn(torch.autograd.Function):
    """MLP.fn(x).squeeze(-1) on the library's kernels: forward tg_decoder_fwd (the three layers in one launch; it keeps
    the pre-activations when a gradient is wanted), backward tg_decoder_bwd (the six weight gradients, deterministic, and
    dx when x needs one); the dropout masks are regenerated from `key`, not stored."""

    @staticmethod
    def forward(ctx, x, p, key, *params):
        x = x.contiguous()
        params = tuple(t.contiguous() for t in params)
        n = x.shape[0]
        y = torch.empty(n, dtype=torch.float32, device=x.device)
        want = any(ctx.needs_input_grad)
        z1 = torch.empty(n, 80, dtype=torch.float32, device=x.device) if want else None
        z2 = torch.empty(n, 10, dtype=torch.float32, device=x.device) if want else None
        decoder_forward(params, x, y, p, key, z1, z2)
        if want:
            ctx.save_for_backward(x, z1, z2, key if p > 0 else None, *params)
            ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z1, z2, key, *params = ctx.saved_tensors
        dy = dy.contiguous().float()
        n, d = x.shape
        grads = tuple(torch.empty_like(t) for t in params)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        nbytes = int(lib.tg_decoder_bwd_workspace_bytes(n, d))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
        w, g = _decoder_struct(params), _decoder_struct(grads)
        check(lib.tg_decoder_bwd(n, ptr(x), d, C.byref(w), float(ctx.p), ptr(key), ptr(z1), ptr(z2), ptr(dy), C.byref(g),
                                 ptr(dx), ptr(ws), ws.numel(), stream_ptr(x.device)), 'tg_decoder_bwd')
        return (dx, None, None) + tuple(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[3:]))


class MLP(nn.Module):
    """The node-classification decoder: fn = Linear(dim, 80) -> ReLU -> Dropout -> Linear(80, 10) -> ReLU -> Dropout ->
    Linear(10, 1), output squeezed (the reference's layout: state_dict keys fn.0.*, fn.3.*, fn.6.*).  A 2-D float32
    input on the GPU with dim a multiple of four (at most 512) runs the three layers as one kernel, under autograd too;
    anything else runs `fn` on plain torch, as MergeLayer does.  Dropout masks come from the library's counter-based
    generator: the module owns its {seed, counter} state (seeded from torch.initial_seed(), as the training step's is)
    and advances it by one for every training forward."""

    def __init__(self, dim: int, dropout: float = 0.3):
        super().__init__()
        self.fn = nn.Sequential(
            nn.Linear(dim, 80), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(80, 10), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(10, 1)
        )
        self._rng = None  # device int64 {seed, counter} (not part of the state dict, as in the reference)

    def params(self):
        f = self.fn
        return (f[0].weight, f[0].bias, f[3].weight, f[3].bias, f[6].weight, f[6].bias)

    def kernel_takes(self, d: int, device: torch.device) -> bool:
        """do rows of width d on `device` take the library's kernels?"""
        w = self.fn[0].weight
        return (device.type == 'cuda' and w.device == device and w.dtype == torch.float32 and w.shape[1] == d
                and d % 4 == 0 and d <= DECODER_MAX_D)

    def hip_ok(self, x: Tensor) -> bool:
        """does the forward of x take the library's kernels?"""
        return x.dim() == 2 and x.dtype == torch.float32 and self.kernel_takes(x.shape[1], x.device)

    def dropout_p(self):
        """the dropout probability of this forward (0 in eval()); None: the two sites differ (the kernel has one)"""
        p1, p2 = float(self.fn[2].p), float(self.fn[5].p)
        if not self.training:
            return 0.0
        return p1 if p1 == p2 else None

    def _next_key(self, device) -> Tensor:
        """this forward's {seed, counter}, and the counter advanced for the next one (device-side: no host sync)"""
        if self._rng is None or self._rng.device != device:
            self._rng = torch.tensor([torch.initial_seed() & (2 ** 63 - 1), 0], dtype=torch.int64, device=device)
        key = self._rng.clone()
        self._rng[1:].add_(1)
        return key

    def forward(self, x):
        p = self.dropout_p()
        if p is None or not self.hip_ok(x):
            return self.fn(x).squeeze(dim=-1)  # CPU tensors, widths the kernel does not take: plain torch
        key = self._next_key(x.device) if p > 0 else None
        return _DecoderFn.apply(x, p, key, *self.params())
