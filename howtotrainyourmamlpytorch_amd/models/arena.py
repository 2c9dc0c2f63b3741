"""Flat fast-weight arena.

The reference carries inner-loop fast weights as a nested name->tensor dict
(``meta_neural_network_architectures.py:11-38``) and updates them tensor by
tensor.  MI355X-first design instead lays every inner-loop-adapted
parameter out in **one contiguous fp32 buffer** per task batch:

* ``theta`` (the meta-learned initialization) is a single ``[P]`` parameter;
* per iteration the fast weights are one ``[T, P]`` tensor (``T`` = tasks
  resident on this GPU), so
* ``autograd.grad`` of the support loss returns ONE ``[T, P]`` tensor,
* the LSLR update is ONE fused elementwise kernel over ``[T, P]``
  (reference: a Python loop over ~10 tensors,
  ``inner_loop_optimizers.py:99-113``),
* the outer meta-gradient all-reduce is ONE flat RCCL bucket.

Layers see the arena through zero-copy views produced by :meth:`views`.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch


@dataclass(frozen=True)
class ParamSpec:
    name: str            # reference-style dotted name, e.g. layer_dict.conv0.conv.weight
    shape: Tuple[int, ...]
    offset: int          # element offset into the flat arena
    numel: int
    slot: int            # LSLR slot id (one learnable per-step LR per spec)


class _ArenaViewsFn(torch.autograd.Function):
    """arena [T, P] -> the per-parameter views (zero-copy, as plain slicing
    gives them).  Backward: the view gradients written side by side into one
    [T, P] tensor by ``_ArenaScatterFn`` — one launch.  A view without a
    gradient stays absent (a zero range in the kernel), never a tensor."""

    @staticmethod
    def forward(ctx, pa, arena):
        ctx.pa = pa
        ctx.set_materialize_grads(False)
        return tuple(pa._slices(arena))

    @staticmethod
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return None, None
        return None, _ArenaScatterFn.apply(ctx.pa, *grads)


class _ArenaScatterFn(torch.autograd.Function):
    """Per-parameter gradients [T, *shape] (None = absent) -> [T, P].
    Linear, and the adjoint of slicing: its backward hands out the slices of
    the incoming [T, P] gradient (views, no kernel), through
    ``_ArenaViewsFn`` again where that gradient is itself differentiated —
    the two Functions are each other's backward, at every order."""

    @staticmethod
    def forward(ctx, pa, *grads):
        from .. import ops
        ctx.pa = pa
        ctx.present = [g is not None for g in grads]
        ctx.set_materialize_grads(False)
        slots = [i for i, g in enumerate(grads) if g is not None]
        T = grads[slots[0]].shape[0]
        return ops.hip_ext().arena_scatter(
            [grads[i] for i in slots], slots,
            [s.offset for s in pa.specs], [s.numel for s in pa.specs],
            T, pa.numel)

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return (None,) * (1 + len(ctx.present))
        pa = ctx.pa
        vs = (_ArenaViewsFn.apply(pa, gout) if pa._native_grad(gout)
              else pa._slices(gout))
        return (None,) + tuple(v if p else None
                               for v, p in zip(vs, ctx.present))


class ParamArena:
    def __init__(self, named_shapes: Sequence[Tuple[str, Tuple[int, ...]]]):
        self.specs: List[ParamSpec] = []
        off = 0
        for slot, (name, shape) in enumerate(named_shapes):
            n = 1
            for s in shape:
                n *= int(s)
            self.specs.append(ParamSpec(name, tuple(int(s) for s in shape), off, n, slot))
            off += n
        self.numel = off
        self._by_name = {s.name: s for s in self.specs}

    @property
    def num_slots(self) -> int:
        return len(self.specs)

    def spec(self, name: str) -> ParamSpec:
        return self._by_name[name]

    def names(self) -> List[str]:
        return [s.name for s in self.specs]

    def slot_index(self, device=None, dtype=torch.long) -> torch.Tensor:
        """[P] tensor mapping each arena element to its LSLR slot — used to
        gather the per-element learning-rate vector for the fused update."""
        idx = torch.empty(self.numel, dtype=dtype)
        for s in self.specs:
            idx[s.offset:s.offset + s.numel] = s.slot
        return idx.to(device) if device is not None else idx

    def pack(self, named: Dict[str, torch.Tensor]) -> torch.Tensor:
        """dict of [shape] tensors -> flat [P] (fp32)."""
        flat = torch.empty(self.numel, dtype=torch.float32)
        for s in self.specs:
            flat[s.offset:s.offset + s.numel] = named[s.name].detach().reshape(-1).float()
        return flat

    def _slices(self, arena: torch.Tensor) -> List[torch.Tensor]:
        """[T, P] -> the per-parameter views [T, *shape], in spec order."""
        T = arena.shape[0]
        return [arena[:, s.offset:s.offset + s.numel].view(T, *s.shape)
                for s in self.specs]

    def _native_grad(self, arena: torch.Tensor) -> bool:
        """Whether views() of this [T, P] arena goes through the Function
        pair with the one-launch gradient (``arena_scatter``): an fp32 arena
        that requires grad, on the GPU, with the extension loaded, at most
        32 parameters (the kernel's table), and MAML355_ARENA_SCATTER=1.
        Opt-in for now: every gradient it was compared on has the bits of
        autograd's own slice backward, but the flagship's deterministic
        output dump moves from the second training step on;
        unset or 0 is the slice backward."""
        if not (arena.is_cuda and arena.requires_grad
                and arena.dtype == torch.float32
                and len(self.specs) <= 32
                and os.environ.get("MAML355_ARENA_SCATTER", "0") == "1"):
            return False
        from .. import ops
        return ops.hip_ext() is not None

    def views(self, arena: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Zero-copy per-parameter views.

        arena [P]   -> name -> [*shape]
        arena [T,P] -> name -> [T, *shape]

        With MAML355_ARENA_SCATTER=1 a ``[T, P]`` arena that requires grad
        on the GPU gets its views from ``_ArenaViewsFn``: the same views, whose gradient is one
        ``arena_scatter`` launch instead of a zero-filled ``[T, P]`` tensor
        per view and their sum.  The views of such an arena must not be
        written in place (nothing does: fast weights are replaced by
        ``lslr_update``, never updated); autograd refuses such a write.
        """
        out: Dict[str, torch.Tensor] = {}
        if arena.dim() == 1:
            for s in self.specs:
                out[s.name] = arena[s.offset:s.offset + s.numel].view(*s.shape)
        elif arena.dim() == 2:
            if self._native_grad(arena):
                vs = _ArenaViewsFn.apply(self, arena)
            else:
                vs = self._slices(arena)
            for s, v in zip(self.specs, vs):
                out[s.name] = v
        else:
            raise ValueError("arena must be [P] or [T, P], got %s" % (arena.shape,))
        return out

    def unpack(self, arena: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {k: v.clone() for k, v in self.views(arena).items()}
