"""Query side of ``StreamPETRHead`` on the GPU: from the temporal memory bank to the decoder's inputs.

:class:`HeadQueries` is lines :641-652 of ``StreamPETRHead.forward`` (``dense_heads/streampetr_head.py``) with ``temporal_alignment`` (:424-453) at inference
time (``prepare_for_dn`` returns the learned points repeated per sample and no mask): ``reference_points``, ``query_embedding(pos2posemb3d(.))``, ``tgt``, both
``MLN(180)`` over the NeRF-encoded ego motion, ``time_embedding(pos2posemb1d(.))`` and the concatenation of the ``num_propagated`` newest memory entries behind
the learned queries.  It sits between :meth:`toc3d_amd.TemporalMemory.pre_update_memory` and :class:`toc3d_amd.PETRTemporalTransformer`; its
``reference_points`` and ``rec_ego_pose`` go on to :class:`toc3d_amd.HeadOutputs` and :meth:`toc3d_amd.TemporalMemory.post_update_memory`.  Parameters live under the
reference's names (``reference_points``, ``query_embedding.{0,2}``, ``time_embedding.{0,1}``, ``ego_pose_pe`` / ``ego_pose_memory`` ``.{reduce.0,gamma,beta}``), so that
slice of a ``pts_bbox_head.*`` checkpoint loads strictly.  ``pseudo_reference_points`` stays with :class:`toc3d_amd.TemporalMemory`.

Per frame (``csrc/head_queries.hip``, ``include/toc3d.h``), on the B * memory_len memory entries only: ``toc3d_head_query_inputs`` (the three GEMM A operands and the
tail of ``reference_points``) -> ``query_embedding.0`` -> ReLU -> ``query_embedding.2``; ONE N = 512 GEMM for ``ego_pose_pe.reduce.0 | ego_pose_memory.reduce.0`` ->
ReLU -> one N = 512 GEMM per MLN for ``gamma | beta``; ``time_embedding.0``; ``toc3d_head_query_combine`` (LayerNorms, MLNs, the sum, and the concatenation as
store addresses): ten launches, recorded once per (shape, input buffers) and replayed with one C call.  The learned queries' half of ``query_pos`` / ``tgt`` depends
on weights only: it is computed once with the same kernels and GEMMs (derived state, dropped by ``load_state_dict`` and ``.to()``).  No CPU path.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from . import gemm, lib
from .gemm import DEFAULT_PRECISION
from .staged import MLN, StagedModule, dim_t, host_range, require_cuda          # (dim_t: re-exported, tests and a tool read it from here)

_MAX_STATES = 8                      # recorded plans kept per module: a plan names its input buffers (a TemporalMemory alternates between two banks)


class HeadQueries(StagedModule):
    _NAME, _RUNS, _SUPPORTED = "toc3d_amd.HeadQueries", "the query side runs", ("bf16", "fp32x3", "fp32")
    _DERIVED = dict(StagedModule._DERIVED, _fresh=None)

    def __init__(self, num_query=644, memory_len=1024, num_propagated=256, embed_dims=256, with_ego_pos=True,
                 pc_range: Sequence[float] = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), precision=DEFAULT_PRECISION, launch_mode="plan"):
        super().__init__()
        if embed_dims != 256:
            raise NotImplementedError(f"{self._NAME}: embed_dims={embed_dims} is not implemented: the reference fixes 256 (pos2posemb3d yields 3 * 128 = embed_dims * 3 // 2 "
                                      "columns, pos2posemb1d 256, MLN(180) has f_dim 256)")
        self._init_staged(precision, launch_mode)
        if not (num_query > 0 and memory_len > 0 and 0 <= num_propagated <= memory_len):
            raise ValueError(f"{self._NAME}: num_query={num_query}, memory_len={memory_len}, num_propagated={num_propagated} (need 0 <= num_propagated <= memory_len)")
        E = embed_dims
        self.num_query, self.memory_len, self.num_propagated, self.embed_dims, self.with_ego_pos = num_query, memory_len, num_propagated, E, bool(with_ego_pos)
        self.reference_points = nn.Embedding(num_query, 3)                                                  # :277
        self.query_embedding = nn.Sequential(nn.Linear(E * 3 // 2, E), nn.ReLU(), nn.Linear(E, E))          # :282-286
        self.time_embedding = nn.Sequential(nn.Linear(E, E), nn.LayerNorm(E))                               # :290-293
        if self.with_ego_pos:                                                                               # :296-298
            self.ego_pose_pe, self.ego_pose_memory = MLN(180, E), MLN(180, E)
        self._pc = host_range(pc_range)
        self._unit = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], dtype=torch.float32)    # the learned points are already normalised: (p - 0) / 1 = p
        self.pc_range = [float(v) for v in pc_range]
        self.fresh_builds = 0                       # how often the learned queries' half was computed (once per set of weights and device)

    def init_weights(self):                         # :303
        nn.init.uniform_(self.reference_points.weight.data, 0, 1)
        self._drop_derived()

    # ------------------------------------------------------------------------------------------------------------------------------
    def _pack(self, pk):
        cat = pk.linear                                            # (fp32x3: weights and the input kernel's rows as (hi, lo) planes)
        P = dict(dts=pk.dts, qe0=cat(self.query_embedding[0]), qe2=cat(self.query_embedding[2]), te=cat(self.time_embedding[0]),
                 te_ln=pk.layernorm(self.time_embedding[1]), dimt3=dim_t(128).to(pk.dev), dimt1=dim_t(256).to(pk.dev))
        if self.with_ego_pos:
            pe, mem = self.ego_pose_pe, self.ego_pose_memory
            P.update(red=cat(pe.reduce[0], mem.reduce[0]), gb_pe=cat(pe.gamma, pe.beta), gb_mem=cat(mem.gamma, mem.beta))
        return P

    def _scratch(self, M, dev):
        """The intermediate buffers of ``M`` rows."""
        tdt, f = self._packed["dts"].torch, torch.float32
        z = lambda c, d: torch.zeros(M, c, dtype=d, device=dev)
        S = dict(pos3d=z(384, tdt), t1d=z(256, tdt), h1=z(256, tdt), qe=z(256, f), te=z(256, f))
        if self.with_ego_pos:
            S.update(nerf=z(192, tdt), red=z(512, tdt), gb_pe=z(512, f), gb_mem=z(512, f))
        return S

    def _launches(self, S, src, dst, B, n, np_):
        """The launch sequence on ``B * n`` rows (eager or being recorded).  ``src``: (tensor or pointer, sample stride) of reference points, velo, f64 timestamps,
        ego poses, embeddings and the host pc_range; ``dst``: the store addresses of ``toc3d_head_query_combine`` and the reference-point tail."""
        P, E, M = self._packed, self.embed_dims, B * n
        dts, s, ego = P["dts"], lib.stream_ptr(), self.with_ego_pos
        (ref, ref_s), (vel, vel_s), (ts, ts_s), (pose, pose_s), (emb, emb_s), pc = src

        def linear(a, wb, out, N, K, lda, ldo, f32_out, planes):
            self._linear(a, wb, out, M, N, K, f32_out=f32_out, lda=lda, ldo=ldo, a_planes=planes and dts.x3p)

        lib.call("toc3d_head_query_inputs", dts.rows, ref, ref_s, vel, vel_s, ts, ts_s, pose, pose_s, pc, P["dimt3"], P["dimt1"], S["pos3d"], 384,
                 S["nerf"] if ego else None, 192, S["t1d"], 256, dst["ref_tail"], dst["ref_stride"], B, n, np_, E, s)
        linear(S["pos3d"], P["qe0"], S["h1"], E, 384, 384, E, False, True)                                  # query_embedding.0
        lib.call("toc3d_relu_inplace", dts.act, S["h1"], S["h1"].numel(), s)
        linear(S["h1"], P["qe2"], S["qe"], E, E, E, E, True, False)                                         # query_embedding.2
        if ego:
            linear(S["nerf"], P["red"], S["red"], 2 * E, 192, 192, 2 * E, False, True)                      # ego_pose_pe.reduce.0 | ego_pose_memory.reduce.0
            lib.call("toc3d_relu_inplace", dts.act, S["red"], S["red"].numel(), s)
            linear(S["red"], P["gb_pe"], S["gb_pe"], 2 * E, E, 2 * E, 2 * E, True, False)                   # ego_pose_pe.gamma | beta
            linear(S["red"].data_ptr() + E * S["red"].element_size(), P["gb_mem"], S["gb_mem"], 2 * E, E, 2 * E, 2 * E, True, False)       # ego_pose_memory.gamma | beta
        linear(S["t1d"], P["te"], S["te"], E, E, E, E, True, True)                                          # time_embedding.0
        w, b, eps = P["te_ln"]
        lib.call("toc3d_head_query_combine", S["qe"], E, S["gb_pe"] if ego else None, 2 * E, S["te"], E, w, b, eps, emb, emb_s, E, S["gb_mem"] if ego else None, 2 * E,
                 dst["qpos_tail"], dst["tail_stride"], dst["tgt_tail"], dst["tail_stride"], E, dst["temp_pos"], dst["temp_mem"], E, B, n, np_, E, s)

    def _build_fresh(self, dev):
        """``query_pos`` and ``tgt`` of the ``num_query`` learned points (:649-650, :433-436, :442): the memory half's launch sequence on the learned points with zero
        velocity and timestamp, identity poses and zero embeddings (``tgt`` is then the MLN's ``beta`` branch: the LayerNorm of a zero row is zero)."""
        nq, E, f = self.num_query, self.embed_dims, torch.float32
        S = self._scratch(nq, dev)
        z = lambda *s, d=f: torch.zeros(*s, dtype=d, device=dev)
        ref = self.reference_points.weight.detach().to(device=dev, dtype=f).contiguous()
        pose = torch.eye(4, dtype=f, device=dev).repeat(nq, 1, 1)
        vel, ts, emb, qpos, tgt = z(nq, 2), z(nq, d=torch.float64), z(nq, E), z(nq, E), z(nq, E)
        src = ((ref, nq * 3), (vel, nq * 2), (ts, nq), (pose, nq * 16), (emb, nq * E), self._unit)
        dst = dict(ref_tail=None, ref_stride=0, qpos_tail=None, tgt_tail=None, tail_stride=0, temp_pos=qpos, temp_mem=tgt)
        self._launches(S, src, dst, 1, nq, 0)
        torch.cuda.current_stream().synchronize()              # the scratch buffers go out of scope
        self.fresh_builds += 1
        return dict(query_pos=qpos, tgt=tgt, reference_points=ref)

    def _alloc(self, key, dev):
        """Scratch rows and ONE flat buffer that holds the six outputs; its learned-query rows and ``rec_ego_pose`` are written here, once."""
        if self._fresh is None:
            self._fresh = self._build_fresh(dev)
        B, n = key
        nq, np_, E = self.num_query, self.num_propagated, self.embed_dims
        Q, nt = nq + np_, n - np_
        sizes = dict(tgt=B * Q * E, query_pos=B * Q * E, temp_memory=B * nt * E, temp_pos=B * nt * E, rec_ego_pose=B * Q * 16, reference_points=B * Q * 3)
        flat = torch.zeros(sum(gemm.round_up(v, 4) for v in sizes.values()), dtype=torch.float32, device=dev)
        off, o = {}, 0
        for k, v in sizes.items():
            off[k] = (o, v)
            o += gemm.round_up(v, 4)
        view = lambda t, k, *shape: t[off[k][0]:off[k][0] + off[k][1]].view(*shape)
        shapes = dict(tgt=(B, Q, E), query_pos=(B, Q, E), reference_points=(B, Q, 3), temp_memory=(B, nt, E), temp_pos=(B, nt, E), rec_ego_pose=(B, Q, 4, 4))
        out = {k: view(flat, k, *shp) for k, shp in shapes.items()}
        for k in ("tgt", "query_pos", "reference_points"):
            out[k][:, :nq] = self._fresh[k]
        out["rec_ego_pose"][:] = torch.eye(4, dtype=torch.float32, device=dev)
        tail = lambda t, w: t.data_ptr() + nq * w * 4
        dst = dict(ref_tail=tail(out["reference_points"], 3) if np_ else None, ref_stride=Q * 3, qpos_tail=tail(out["query_pos"], E) if np_ else None,
                   tgt_tail=tail(out["tgt"], E) if np_ else None, tail_stride=Q * E, temp_pos=out["temp_pos"] if nt else None,
                   temp_mem=out["temp_memory"] if nt else None)
        return dict(S=self._scratch(B * n, dev), flat=flat, shapes=shapes, view=view, dst=dst)

    @staticmethod
    def _strided(t):
        """(tensor, sample stride in elements) of a bank tensor (B, n, ...): dense samples at any stride -- a view of a capacity buffer goes in as it is."""
        per = t[0].numel()
        if not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < per):
            t = t.contiguous()                              # a layout that (sample stride, dense rows) cannot express
        return t, (t.stride(0) if t.shape[0] > 1 else per)

    @torch.no_grad()
    def forward(self, memory_embedding, memory_reference_point, memory_timestamp, memory_egopose, memory_velo):
        """The five bank tensors as :class:`toc3d_amd.TemporalMemory` exposes them after ``pre_update_memory``: f32 (B, memory_len, 256 / 3 / 4, 4 / 2) and the f64
        timestamps (B, memory_len, 1); for B > 1 they are strided views of capacity buffers and are read through their sample stride (no copy).

        Returns ``(tgt, query_pos, reference_points, temp_memory, temp_pos, rec_ego_pose)`` as ``temporal_alignment`` does: ``tgt``, ``query_pos`` (B, num_query +
        num_propagated, 256), ``reference_points`` (B, ., 3), ``temp_memory``, ``temp_pos`` (B, memory_len - num_propagated, 256), ``rec_ego_pose`` (B, ., 4, 4)
        identities -- all f32 and freshly allocated every call (views of one new buffer; none aliases a workspace or an input).  The reference sizes
        ``rec_ego_pose`` from ``query_pos`` after the concatenation (:447, :449) and so returns ``num_propagated`` surplus identities that nothing can index; they
        are not returned here."""
        ins = (memory_embedding, memory_reference_point, memory_timestamp, memory_egopose, memory_velo)
        require_cuda(self._NAME, *ins)
        B, n, E = memory_embedding.shape[0], self.memory_len, self.embed_dims
        if (tuple(memory_embedding.shape) != (B, n, E) or tuple(memory_reference_point.shape) != (B, n, 3) or tuple(memory_timestamp.shape) != (B, n, 1)
                or tuple(memory_egopose.shape) != (B, n, 4, 4) or tuple(memory_velo.shape) != (B, n, 2)):
            raise ValueError(f"{self._NAME}: bank tensors {[tuple(t.shape) for t in ins]} do not fit memory_len={n}, embed_dims={E}")
        if memory_timestamp.dtype != torch.float64 or any(t.dtype != torch.float32 for t in (memory_embedding, memory_reference_point, memory_egopose, memory_velo)):
            raise TypeError(f"{self._NAME}: the bank is f32 with f64 timestamps (as toc3d_amd.TemporalMemory keeps it), got {[t.dtype for t in ins]}")
        dev = memory_embedding.device
        with torch.cuda.device(dev):
            W = self._workspace((B, n), dev)
            emb, ref, ts, pose, vel = (self._strided(t.detach()) for t in ins)
            src = (ref, vel, ts, pose, emb, self._pc)
            # a recorded plan names its input buffers: one state per (shape, buffers, strides); the bank alternates between two
            key = (B, n) + tuple((t.data_ptr(), st) for t, st in (ref, vel, ts, pose, emb))
            self._run(key, lambda: self._launches(W["S"], src, W["dst"], B, n, self.num_propagated), max_states=_MAX_STATES)
            out = W["flat"].clone()
            o = {k: W["view"](out, k, *shp) for k, shp in W["shapes"].items()}
            return o["tgt"], o["query_pos"], o["reference_points"], o["temp_memory"], o["temp_pos"], o["rec_ego_pose"]

    def forward_from(self, memory):
        """``forward`` on the bank of a :class:`toc3d_amd.TemporalMemory` (after its ``pre_update_memory``)."""
        return self.forward(memory.memory_embedding, memory.memory_reference_point, memory.memory_timestamp, memory.memory_egopose, memory.memory_velo)
