"""What the head's modules share on the host: :class:`StagedModule`, the base of ``HeadTokenEmbedding``, ``HeadQueries``, ``PETRTemporalTransformer`` and
``HeadOutputs`` -- one lane of launches per frame on staged inputs, from weights packed on first use, in per-shape workspaces, replayed from a recorded plan -- and
the small things more than one of them (and the backbone's scorer) builds the same way: the ``MLN`` parameter container, ``dim_t`` and the host copy of a range.

A module on the base keeps what is its own: the config it accepts, its parameter containers, ``_pack(pk)`` (what it packs, with a :class:`toc3d_amd.gemm.Packer`),
``_alloc(key, dev)`` (the buffers of one shape), its launch sequence and the views it returns.  ``CPFPN`` and the backbones own tuning tables and multi-lane frames
and stay on :class:`toc3d_amd.plan.DerivedState` alone: the backbones share their own frame driver (``backbone._BackboneBase._master`` / ``_drive``).  What all of
them share is ``gemm.Packer`` for packing and ``plan.lru`` for the caches of plans and launch states.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import gemm, lib, plan


def require_cuda(name, *tensors, on_device=True):
    """The refusal of anything but device tensors (``on_device=False``: of anything but tensors, for a module that checks shapes before the device)."""
    for t in tensors:                                       # (a plain loop: this runs every frame)
        if not isinstance(t, torch.Tensor) or (on_device and not t.is_cuda):
            raise RuntimeError(f"{name}: inputs must be CUDA/HIP tensors -- the HIP extension is the only compute path (no CPU fallback)")


def host_range(values) -> torch.Tensor:
    """f32 host copy of ``pc_range`` / ``position_range``: the C ABI takes the six values from the host."""
    t = torch.tensor([float(v) for v in values], dtype=torch.float32)
    assert t.numel() == 6
    return t


def dim_t(num_pos_feats: int, temperature: float = 10000) -> torch.Tensor:
    """The reference's expression for ``dim_t`` (``positional_encoding.py:17-18`` / :31-32), on the host: the kernels take the table, they do not recompute it."""
    t = torch.arange(num_pos_feats, dtype=torch.float32)
    return temperature ** (2 * torch.div(t, 2, rounding_mode="floor") / num_pos_feats)


class MLN(nn.Module):
    """Parameter container of the reference's ``MLN`` (``models/utils/misc.py:154-188``); ``reset_parameters``: its zero / one init of gamma and beta, for a module
    that is used as built (the backbone's scorer; the head's modules load theirs)."""

    def __init__(self, c_dim, f_dim, reset_parameters=False):
        super().__init__()
        self.reduce = nn.Sequential(nn.Linear(c_dim, f_dim), nn.ReLU())
        self.gamma, self.beta = nn.Linear(f_dim, f_dim), nn.Linear(f_dim, f_dim)
        if reset_parameters:
            nn.init.zeros_(self.gamma.weight)
            nn.init.zeros_(self.beta.weight)
            nn.init.ones_(self.gamma.bias)
            nn.init.zeros_(self.beta.bias)


class StagedModule(plan.DerivedState, nn.Module):
    _NAME = "toc3d_amd.StagedModule"           # the module's name in its refusals
    _RUNS = "the module runs"                  # ... and what the unsupported-precision refusal says runs in _SUPPORTED
    _SUPPORTED = ()
    # packed weights, workspaces (the split-K ones of gemm.linear included) and recorded plans, which point into both, are derived state
    _DERIVED = dict(_packed=None, _ws={}, _states={}, _sk_ws={}, _sk_ws_old=[])
    _INSTANCE = dict(_pool=[])

    def _init_staged(self, precision, launch_mode="eager"):
        if precision not in self._SUPPORTED:
            raise NotImplementedError(f"{self._NAME}: precision {precision!r} is not implemented; {self._RUNS} in {' or '.join(repr(p) for p in self._SUPPORTED)}")
        assert launch_mode in plan.MODES, launch_mode
        self.precision, self.launch_mode = precision, launch_mode
        self._pool = []
        self._drop_derived()

    def _workspace(self, key, dev):
        """The module's ``_alloc(key, dev)`` for the shape ``key``, once, on the current device ``dev``; before that its ``_pack(gemm.Packer)`` if new weights arrived."""
        if self._packed is None:
            self._packed = self._pack(gemm.Packer(gemm.dtypes(self.precision), dev))
            torch.cuda.current_stream().synchronize()              # the pack launches' temporaries go out of scope
        W = self._ws.get(key)
        if W is None:
            W = self._ws[key] = self._alloc(key, dev)
        return W

    def _run(self, key, launches, mode=None, max_states=None):
        """One frame: ``launches()`` on lane 0, in ``mode`` (default: the module's ``launch_mode``) through ``plan.run_frame`` on ``self._states[key]``.  A module
        whose recorded plans name buffers that are not its own keeps at most ``max_states`` of them, the oldest dropped first (``plan.lru``'s miss)."""
        state = self._states.get(key)                              # (a hit leaves the order alone: here the oldest recording goes first, not the least used)
        if state is None:
            state = plan.lru(self._states, key, dict, max_states)

        def frame(ex):
            with ex.lane(0):
                launches()
        plan.run_frame(state, self.launch_mode if mode is None else mode, 1, frame, self._pool)

    def _linear(self, a, wb, out, M, N, K, *, f32_out=False, relu=False, residual=None, lda=None, ldo=None, a_planes=False):
        """One Linear on ``gemm.linear``, ``wb`` = a packed ``(weight, bias)``: ``out`` in the act dtype (``relu``: through the ReLU epilogue), or f32 rows with
        ``f32_out`` or a ``residual`` (f32 rows, added).  The tile is the query side's rule, ``gemm.small_m_variant``."""
        epi = lib.EPI_RESIDUAL if f32_out or residual is not None else lib.EPI_BIAS_RELU if relu else lib.EPI_BIAS
        gemm.linear(self, epi, a, wb[0], wb[1], out, M, N, K, lda=lda, ldo=ldo, residual=residual, ldr=0 if residual is None else residual.shape[1],
                    a_planes=a_planes, variant=gemm.small_m_variant(M, N, K, residual is not None))
