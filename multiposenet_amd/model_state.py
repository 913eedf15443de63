"""Host-side state of a trainable model, shared by KeypointNet, PersonDetectorNet and PoseResidualNet.

Every trainable variable lives in ONE flat f32 arena, and its gradient and the two Adam slots in arenas of the same layout:
Adam is one fused pass and the data-parallel all-reduce sees one buffer. The batch-norm moving statistics live in a second
arena. `vars`, `grads` and `stats` are named views over them, keyed and ordered by the reference's variable names, whatever
the arenas' layout order; checkpoints go by those names.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from ._lib import ACT_RELU


def is_trainable(name):
    return not (name.endswith("moving_mean") or name.endswith("moving_variance"))


def resolve_device(device):
    """torch.device of `device`; a bare "cuda" is the current device (methods run under _lib.device_guarded with it)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class _Arena:
    """Flat f32 device arena with named, 16-byte aligned views."""

    def __init__(self, shapes, device):
        self.offsets = OrderedDict()
        off = 0
        for name, shape in shapes.items():
            n = int(np.prod(shape))
            self.offsets[name] = (off, n, tuple(shape))
            off += (n + 3) // 4 * 4
        self.size = off
        self.device = device

    def new(self):
        return torch.zeros(self.size, dtype=torch.float32, device=self.device)

    def views(self, flat):
        return OrderedDict((k, flat[o:o + n].view(shape)) for k, (o, n, shape) in self.offsets.items())


class _Conv:
    """One dense conv: reference variable view (+ gradient view) and packed MFMA operands. `as1x1`: a 3x3 HWIO kernel used as
    the [1,1,9*Cin,Cout] matrix behind mpn_patchify3x3s2 (the detector's stride-2 convolutions). `pad_cout`: the operands
    are packed from a staging copy with zero columns up to that many output channels (the kernels want multiples of 8)."""

    def __init__(self, name, w, dw, dtype, as1x1=False, pad_cout=0):
        self.name, self.w, self.dw = name, w, dw
        k, _, cin, cout = w.shape
        self.pad = None
        if pad_cout:
            self.pad = torch.zeros((k, k, cin, pad_cout), dtype=torch.float32, device=w.device)
            self.dpad = torch.zeros_like(self.pad)
            cout = pad_cout
        src = self.pad if self.pad is not None else w
        if as1x1:
            src = src.view(1, 1, k * k * cin, cout)
        self.ksize, self.cin, self.cout = src.shape[0], src.shape[2], src.shape[3]
        self.src = src
        self.refresh_pad()
        self.packed = ops.PackedConv(src, dtype)

    def refresh_pad(self):
        if self.pad is not None:
            self.pad[..., :self.w.shape[3]].copy_(self.w)

    def repack(self):
        if getattr(self, "packed_unused", False):
            return
        self.refresh_pad()
        self.packed.repack()


class ModelState:
    """Mixin: the arenas, their named views, the optimizer's step state and the checkpoint surface of a model. The model sets
    `device` and `dtype`, then calls `_init_state`."""

    # names `load_state_dict(strict=True)` does not know: an error, or (the PRN: its checkpoints may hold Adam slots) skipped
    ignore_unknown = False

    # what `_init_state` creates: the state `share_variables` hands to another instance
    _SHARED = ("_train_arena", "_stat_arena", "theta", "grad", "adam_m", "adam_v", "moving", "vars", "grads", "stats",
               "global_step", "hyper", "_pads", "_version")

    def _init_state(self, shapes, order=None, pads=None):
        """shapes: ordered {reference name: shape as the arenas hold it} (variables and moving statistics); order: the arenas'
        layout order of those names (default: that of `shapes`); pads: {name: (axis, reference size)} of the variables the
        arenas hold wider than the reference (net.internal_shapes)."""
        layout = OrderedDict((k, shapes[k]) for k in (order if order is not None else shapes))
        self._train_arena = _Arena(OrderedDict((k, v) for k, v in layout.items() if is_trainable(k)), self.device)
        self._stat_arena = _Arena(OrderedDict((k, v) for k, v in layout.items() if not is_trainable(k)), self.device)
        self.theta = self._train_arena.new()
        self.grad = self._train_arena.new()
        self.adam_m = self._train_arena.new()
        self.adam_v = self._train_arena.new()
        self.moving = self._stat_arena.new()

        def named(arena, flat):      # (in the reference's order, whatever the arena's)
            v = arena.views(flat)
            return OrderedDict((k, v[k]) for k in shapes if k in v)
        self.vars, self.grads = named(self._train_arena, self.theta), named(self._train_arena, self.grad)
        self.stats = named(self._stat_arena, self.moving)
        self.global_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.hyper = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._pads = dict(pads or {})
        self._version = [0]
        self.convs = []              # the dense convs over the views (_conv), once the model builds its layers

    def share_variables(self, other, *extra):
        """Run on `other`'s variables, statistics, Adam slots and step state (and its attributes named in `extra`)."""
        for a in self._SHARED + extra:
            setattr(self, a, getattr(other, a))

    @property
    def var_version(self):
        """Moves with every mark_variables_changed (shared with the instances that share_variables)."""
        return self._version[0]

    def mark_variables_changed(self):
        """Variables or moving statistics changed: cached inference affines are stale and `var_version` moves (users that
        replay captured device work - inference/detector.py - compare it). Every method of this object that changes them
        calls this; so must whoever changes them from outside: a replayed hipGraph of a train step (train.Trainer.step does),
        a direct write into `vars` / `stats`."""
        self._version[0] += 1
        self._infer_clean = False

    def unpad(self, name, t):
        """The reference-shaped part of an arena view (variable, gradient or Adam slot) of `name` (net.internal_shapes)."""
        if name in self._pads:
            axis, n = self._pads[name]
            return t.narrow(axis, 0, n)
        return t

    def state_dict(self):
        """{reference variable name: numpy array}: the variables, then the moving statistics, in reference shapes."""
        return OrderedDict((k, self.unpad(k, v).detach().cpu().numpy().copy())
                           for k, v in list(self.vars.items()) + list(self.stats.items()))

    def load_state_dict(self, values, strict=True):
        """Copy {reference name: array} into the variables and statistics; a pad is reset to zeros. strict: every variable
        and statistic must be in `values`, and every name of `values` must be the model's (unless `ignore_unknown`)."""
        for k, v in values.items():
            dst = self.vars.get(k, self.stats.get(k))
            if dst is None:
                if strict and not self.ignore_unknown:
                    raise KeyError(f"unknown variable {k}")
                continue
            self._copy_in(k, dst, v)
        if strict:
            missing = [k for k in list(self.vars) + list(self.stats) if k not in values]
            if missing:
                raise KeyError(f"missing variables: {missing[:5]}...")
        self.mark_variables_changed()
        self._variables_loaded()

    def _copy_in(self, name, dst, value, label=None):
        """Copy a reference-shaped array into the arena view `dst` of variable `name` (or of its gradient, an Adam slot);
        the pad is reset to zeros, gamma included (see net.internal_shapes). label: the name in a shape error."""
        v = np.asarray(value, dtype=np.float32)
        if name in self._pads:
            dst.zero_()
            dst = self.unpad(name, dst)
        if tuple(v.shape) != tuple(dst.shape):
            raise ValueError(f"{label or name}: shape {v.shape} != {tuple(dst.shape)}")
        dst.copy_(torch.from_numpy(v))

    def _variables_loaded(self):
        """After load_state_dict: refresh what is derived from the variables - the packed conv operands, once built."""
        if self.convs:
            self.repack_weights()

    def _bn(self, prefix, act=ACT_RELU):
        bn = ops.BNState(self.vars[prefix + "/gamma"], self.vars[prefix + "/beta"], self.stats[prefix + "/moving_mean"],
                         self.stats[prefix + "/moving_variance"], act)
        bn.dgamma, bn.dbeta = self.grads[prefix + "/gamma"], self.grads[prefix + "/beta"]
        bn.name = prefix
        return bn

    def _conv(self, name, **kw):
        c = _Conv(name, self.vars[name], self.grads[name], self.dtype, **kw)
        self.convs.append(c)
        return c
