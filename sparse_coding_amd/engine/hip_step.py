"""Fused CDNA4 training step for SAE ensembles.

Implements the reference's vmapped grad+Adam `step_batch`
(autoencoders/ensemble.py:119-123,175-193 + the signature losses in
sae_ensemble.py / topk_encoder.py / mlp_tests.py) as a pipeline of
hand-written gfx950 HIP kernels (``sparse_coding_amd/ops/hip/sae_kernels.hip``):

  k_row_norms    : per-row ||w|| and 1/max(||w||,1e-8) of the dictionary
  k_enc_fwd      : encoder GEMM -> epilogue by mode: bias+ReLU (0), raw
                   scores for TopK (1), threshold gate (2), reverse
                   bias-subtract (3); + L1 partial, fired counts, optional
                   per-model coef mask (K9) and per-model x stride
  k_dec_fwd      : decoder GEMM (rows scaled by inv-norm) -> residual r
                   (+MSE partial)
  k_gc           : code-grad GEMM -> relu/sign mask + l1 term -> g_pre
                   (+bias-grad column sums); k_gc_thresh adds the gate
                   derivative and gain/scale column-sum grads
  k_grad_w       : batch-contraction GEMMs -> dL/d(W_hat) (and encoder grad)
  k_project_adam : analytic gradient of w/max(||w||,eps) (the in-forward
                   decoder renormalization) + fused Adam; optional separate
                   "used" weights + clamp-derivative mask (positive SAE)
  k_bias_adam    : Adam on any [M,k] vector param (+ L2-decay gradient)
  k_topk_select  : per-row radix top-k + scatter (TopK)
  k_btk_hist/k_btk_write : batch-level radix top-k over many workgroups +
                   scatter + inference-threshold state (BatchTopK)

Fused-step coverage: EVERY trainable signature in the zoo — tied, untied,
masked tied/untied, thresholding, reverse, tied-centered, positive-tied,
TopK, BatchTopK, LISTA, residual-denoising and semilinear.

Structure.  Every step class derives from ``_HipStep``, which owns what
does not depend on the signature: the Adam hyper-parameters, the kernel
configuration resolved once per workspace allocation, the
``grads_phase`` / ``update_phase`` / ``step`` protocol with hipGraph
capture (``GraphReplay``), and the two Adam launch helpers.  A class supplies its workspaces
(``_alloc_workspaces``), its kernel sequence (``_grads``), its
``update_phase`` and its ``_loss_data``.

``HipSAEStep`` (tied, untied, masked, reverse) holds the
transpose-in-staging launch chain ``_chain``: row norms -> enc_fwd ->
dec_fwd -> gc -> the two grad_w GEMMs.  The centered, whitened and positive
steps prepare their input (and dictionary), call that chain and add what is
special to them; the thresholding step shares its weight-grad tail.  The
pre-transposed (``staging="pre"``) pipeline is HipSAEStep's measured
alternative to the chain.  The unrolled/MLP encoders (HipLISTAStep /
HipResidualDenoisingStep / HipSemilinearStep) orchestrate the same MFMA GEMM
kernels with hand-derived backward chains: LISTA fuses all its elementwise
work into GEMM epilogues and one custom pass, the other two run their
elementwise glue as torch ops on persistent workspaces.

Every class replays its step from a captured hipGraph after two eager
steps, except HipResidualDenoisingStep and HipSemilinearStep, which run
eagerly.

All GEMMs run on the exact-f32 MFMA path (v_mfma_f32_32x32x2_f32): fp32 end
to end, the reference's training dtype.  Validated against the
torch/vmap oracle in tests/test_hip_numerics.py.

For multi-GPU DP the step splits at the gradient boundary
(`grads_phase` / `update_phase`) so the RCCL all-reduce of [M,n,d] grads
overlaps with nothing locally but lands between grad GEMMs and Adam.
"""

from __future__ import annotations

import gc
import os
from typing import Optional

import torch

from sparse_coding_amd import ops as _ops
from sparse_coding_amd.models import sae_signatures as sigs
from sparse_coding_amd.ops.kconfig import kernel_config

EPS_NORM = 1e-8


def _identity_centering(buffers) -> bool:
    rot = buffers.get("center_rot")
    scale = buffers.get("center_scale")
    trans = buffers.get("center_trans")
    if rot is None and scale is None and trans is None:
        return True
    d = rot.shape[-1]
    eye = torch.eye(d, device=rot.device, dtype=rot.dtype).expand_as(rot)
    return torch.equal(rot, eye) and bool((scale == 1).all()) and bool((trans == 0).all())


def maybe_make_step(ensemble, required: bool = False) -> Optional["_HipStep"]:
    """Return the fused step for (sig, device, buffers) if one exists.

    On a CUDA device with a supported signature, a missing extension is a
    hard error: GPU runs must not silently fall back to eager."""
    if os.environ.get("SPARSE_CODING_AMD_FORCE_TORCH") == "1":
        return None

    dev = torch.device(ensemble.device) if not isinstance(ensemble.device, torch.device) else ensemble.device
    if dev.type != "cuda":
        if required:
            raise RuntimeError(f"backend='hip' requested but ensemble device is {dev}")
        return None

    from sparse_coding_amd.models.batch_topk import BatchTopKEncoder
    from sparse_coding_amd.models.lista import (
        FunctionalLISTADenoisingSAE,
        FunctionalResidualDenoisingSAE,
    )
    from sparse_coding_amd.models.positive import FunctionalPositiveTiedSAE
    from sparse_coding_amd.models.semilinear import SemiLinearSAE
    from sparse_coding_amd.models.topk import TopKEncoder

    def sae(**flags):
        return lambda ens, ext: HipSAEStep(ens, ext, **flags)

    make = {
        TopKEncoder: HipTopKStep,
        BatchTopKEncoder: HipBatchTopKStep,
        sigs.FunctionalThresholdingSAE: HipThresholdStep,
        sigs.FunctionalReverseSAE: sae(tied=True, reverse=True),
        sigs.FunctionalTiedCenteredSAE: HipCenteredStep,
        FunctionalPositiveTiedSAE: HipPositiveStep,
        FunctionalLISTADenoisingSAE: HipLISTAStep,
        FunctionalResidualDenoisingSAE: HipResidualDenoisingStep,
        SemiLinearSAE: HipSemilinearStep,
        sigs.FunctionalMaskedTiedSAE: sae(tied=True, masked=True),
        sigs.FunctionalMaskedSAE: sae(tied=False, masked=True),
        sigs.FunctionalTiedSAE: sae(tied=True),
        sigs.FunctionalSAE: sae(tied=False),
    }.get(ensemble.sig)
    if make is None:
        if required:
            raise RuntimeError(f"backend='hip' requested but signature {ensemble.sig.__name__} has no fused step yet")
        return None
    if ensemble.sig is sigs.FunctionalTiedSAE and not _identity_centering(ensemble.buffers):
        # general affine whitening-centering (K7): PCA-whitened-input tied
        # SAE (reference sae_ensemble.py:98-132) — tied pipeline on a
        # precomputed per-model whitened input
        make = HipWhitenedStep
    return make(ensemble, _ops.get_extension(required=True))  # loud on GPU


def _announce(on_grads, *tensors):
    if on_grads is not None:
        on_grads(list(tensors))


class GraphReplay:
    """Runs a body eagerly twice, then from a captured hipGraph.

    Owns the static input, the graph, the eager-step count and the enabled
    flag.  ``key()`` (``_HipStep.graph_key``) names what a captured graph
    depends on: first the workspace allocation, then whatever else the body's
    launches hold addresses of.  A changed key drops the graph; a new
    allocation also restarts the eager count.  After two eager calls at the
    current allocation the next call with that batch size captures, then
    replays.  A failed capture, or being disabled, leaves every call eager."""

    def __init__(self, key, enabled: bool, what: str):
        self.key, self.enabled, self.what = key, enabled, what
        self.graph = None
        self.x_static = None
        self.eager_steps = 0
        self._key = None
        self._B = None  # batch size of the last eager call

    def _check_key(self):
        key = self.key()
        if key != self._key:
            self.graph = None
            if self._key is None or key[0] is not self._key[0]:
                self.eager_steps = 0
            self._key = key

    def _capture(self, x, body):
        # No cyclic garbage collection while the stream is capturing: a
        # collection that starts inside the body may finalize GPU objects of
        # earlier owners (graphs, events, communicators), and releasing those
        # is not allowed during a capture; the runtime aborts the process.
        # torch.cuda.graph collects once itself before the capture begins.
        gc_was_on = gc.isenabled()
        try:
            self.x_static = x.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            gc.disable()
            with torch.cuda.graph(g):
                body(self.x_static)
            self.graph = g
        except Exception as e:  # noqa: BLE001 - graphs are an optimization only
            print(f"{self.what} failed ({e}); staying eager")
            self.enabled = False
            self.graph = None
        finally:
            if gc_was_on:
                gc.enable()

    def run(self, x: torch.Tensor, body) -> None:
        """body(x), eagerly or as a replay of its capture."""
        if self.enabled:
            self._check_key()
            if self.graph is None and self.eager_steps >= 2 and self._B == x.shape[0]:
                self._capture(x.contiguous(), body)  # capture does not execute
            if self.graph is not None and self.x_static.shape == x.shape:
                self.x_static.copy_(x)
                self.graph.replay()
                return
        self.graph = None
        body(x)
        self._check_key()  # body allocates at a new batch size: count from here
        self.eager_steps += 1
        self._B = x.shape[0]


class _HipStep:
    """The signature-independent part of a fused step: hyper-parameters,
    kernel configuration, the phase/step protocol with hipGraph capture,
    and the Adam launch helpers."""

    # replay the step from a captured hipGraph after two eager steps
    captures_graph = True
    # staging this class's kernels need; None -> honour the kernel config
    staging = None
    # the parameter whose [M, n, d] shape sizes the step
    dict_key = "decoder"
    # a data-parallel trainer may run the update on row shards (HipSAEStep)
    row_shardable = False

    def __init__(self, ensemble, ext):
        self.ens = ensemble
        self.ext = ext
        W = ensemble.params[self.dict_key]
        self.n_models, self.n_dict, self.d_act = W.shape
        self._dev = W.device

        opt = ensemble.optimizer_kwargs
        self.lr = float(opt.get("lr", 1e-3))
        betas = opt.get("betas", (0.9, 0.999))
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.eps = float(opt.get("eps", 1e-8))
        name = getattr(ensemble.optimizer_func, "__name__", "adam")
        if name != "adam":
            raise RuntimeError(f"fused HIP step supports adam only, got {name}")

        l1 = ensemble.buffers.get("l1_alpha")  # TopK has no L1 term
        if l1 is not None:
            l1 = l1.detach().to(self._dev, torch.float32).reshape(self.n_models).contiguous()
        self.l1_alpha = l1
        self.zero_decay = torch.zeros(self.n_models, device=self._dev)

        # persistent workspaces, sized lazily on first batch
        self._B = None
        self._allocation = None
        # hipGraph capture of the whole step (single-GPU path): replayed
        # after 2 eager warmup steps; disabled via SPARSE_CODING_AMD_NO_GRAPH=1
        self._replay = GraphReplay(
            self.graph_key, self.captures_graph and os.environ.get("SPARSE_CODING_AMD_NO_GRAPH") != "1",
            "[hip_step] hipGraph capture")

    # -- workspace management -------------------------------------------------
    def _empty(self, *shape):
        return torch.empty(shape, device=self._dev, dtype=torch.float32)

    def _zeros(self, *shape):
        return torch.zeros(shape, device=self._dev, dtype=torch.float32)

    def _ones(self, *shape):
        return torch.ones(shape, device=self._dev, dtype=torch.float32)

    def _alloc(self, B: int):
        kc = kernel_config()
        if self.staging is not None:
            kc["staging"] = self.staging
        if kc["staging"] == "pre" and B % 4 != 0:
            # the pre-transposed operands xT [d, B] / rT [M, d, B] have leading
            # dimension B and are staged as float4: a ragged batch (the last
            # one of a chunk) runs the transpose-in-staging chain instead.
            # Resolved here, once per allocation, so the workspaces, the launch
            # chain and a later graph capture all see the same choice.
            kc["staging"] = "t"
        self.kc = kc
        # tile parameters, resolved once: per-kernel overrides fall back to
        # the global tile depth / width
        self.bk, self.prio, self.bn = kc["bk"], kc["prio"], kc["bn"]
        self.bn_enc = kc["bn_enc"] or self.bn
        self.bk_dec = kc["bk_dec"] or self.bk
        self.bk_gw = kc["bk_grad_w"] or self.bk
        self._alloc_workspaces(B)
        self._B = B
        self._allocation = object()

    def graph_key(self) -> tuple:
        """What a captured graph of this step depends on: the workspace
        allocation first, then any other addresses its launches hold."""
        return (self._allocation,)

    @property
    def use_graph(self) -> bool:
        return self._replay.enabled

    @use_graph.setter
    def use_graph(self, on: bool):
        self._replay.enabled = on

    @property
    def _graph(self):
        return self._replay.graph

    def _alloc_workspaces(self, B: int):
        raise NotImplementedError

    # -- phases ---------------------------------------------------------------
    def grads_phase(self, x: torch.Tensor, on_grads=None):
        """Forward + backward: fills the gradient workspaces and loss parts.

        on_grads: optional callback(list_of_tensors) fired as gradient
        tensors become final — used by the DP trainer to launch RCCL
        all-reduces that overlap the remaining grad GEMMs.  Over one call it
        is handed every tensor of dp_grad_tensors() exactly once (whole, or
        as disjoint slices along dim 0).
        """
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)
        self._grads(x.contiguous(), B, on_grads)
        return B

    def _grads(self, x: torch.Tensor, B: int, on_grads):
        raise NotImplementedError

    def update_phase(self, B: int):
        raise NotImplementedError

    def _loss_data(self, B: int):
        raise NotImplementedError

    def dp_grad_tensors(self):
        """Tensors to all-reduce for data parallelism (average across ranks)."""
        raise NotImplementedError

    @property
    def codes(self):
        """The [M, B, n] codes of the last step (returned as aux["c"])."""
        return self.c

    def _mse_l1_loss(self, B: int, l1_sum):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        l1 = self.l1_alpha * l1_sum / B
        return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}

    # -- Adam launches --------------------------------------------------------
    def _begin_update(self):
        st = self.ens.optim_states
        st["step"] += 1.0
        return st["step"]

    def _param_state(self, key):
        """(param, mu, nu) at a key path: "encoder" or ("encoder_layers", l, "W")."""
        st = self.ens.optim_states
        p, mu, nu = self.ens.params, st["mu"], st["nu"]
        for k in (key,) if isinstance(key, str) else key:
            p, mu, nu = p[k], mu[k], nu[k]
        return p, mu, nu

    def _adam_matrix(self, key, grad, step_no, project, n_per_model=None, lr_mult=None,
                     w_used=None, clamp_mask=False, eps_norm=EPS_NORM, rows=None):
        """Adam on a matrix parameter; project=True first pushes the gradient
        through the in-forward row renormalization (k_project_adam).

        rows=(g0, k) updates rows [g0, g0+k) of the flattened [M*n, d]
        parameter from a [k, d] gradient shard (data-parallel rs_ag): the
        launch sees one model of k rows with the first step counter."""
        W, mu, nu = self._param_state(key)
        norms = self.norms
        if rows is not None:
            sl = slice(rows[0], rows[0] + rows[1])
            W, mu, nu = (t.reshape(-1, t.shape[-1])[sl] for t in (W, mu, nu))
            norms, lr_mult = norms.reshape(-1)[sl], lr_mult.reshape(-1)[sl]
            step_no, n_per_model = step_no.reshape(-1)[0:1], rows[1]
        self.ext.project_adam(W, grad, norms, mu, nu, step_no, n_per_model or self.n_dict,
                              self.lr, self.beta1, self.beta2, self.eps, eps_norm, project,
                              w_used=w_used, clamp_mask=clamp_mask, lr_mult=lr_mult)

    def _adam_vector(self, key, grad, step_no, decay=None, lr_mult=None):
        """Adam on an [M, k] vector parameter (+ L2-decay gradient)."""
        v, mu, nu = self._param_state(key)
        self.ext.bias_adam(v, grad, self.zero_decay if decay is None else decay, mu, nu, step_no,
                           self.lr, self.beta1, self.beta2, self.eps, lr_mult=lr_mult)

    # -- public ---------------------------------------------------------------
    def step(self, minibatches: torch.Tensor, expand_dims: bool = True):
        if not expand_dims:
            raise NotImplementedError("per-model batches not supported by the HIP step")
        self._replay.run(minibatches, lambda x: self.update_phase(self.grads_phase(x)))
        return self._loss_data(minibatches.shape[0]), {"c": self.codes}


class HipSAEStep(_HipStep):
    """Workspaces + kernel-sequence launcher for the plain SAE family:
    tied, untied, masked and reverse."""

    dict_key = "encoder"

    def __init__(self, ensemble, ext, tied: bool, masked: bool = False, reverse: bool = False):
        super().__init__(ensemble, ext)
        self.tied = tied
        self.masked = masked
        # reverse SAE (sae_ensemble.py:447-503): code = pre * [pre+b > 0],
        # |code| in the L1, sign-aware backward, NO bias gradient from the
        # code path (only the L2-decay term moves the bias)
        self.reverse = reverse
        if reverse:
            self.staging = "t"  # the reverse epilogues exist only there

        p = ensemble.params
        if not tied:
            assert p["decoder"].shape == p["encoder"].shape

        dev = self._dev
        b = ensemble.buffers
        bd = b.get("bias_decay")
        # the masked signatures carry a bias_decay buffer but never apply it
        # (reference sae_ensemble.py:347-373,425-444) — force zero
        if bd is None or masked:
            bd = torch.zeros(self.n_models, device=dev)
        self.bias_decay = bd.detach().to(dev, torch.float32).reshape(self.n_models).contiguous()
        self.dict_sizes = None
        if masked:
            # K9: coefficient columns >= dict_size[m] are masked to zero in
            # the encoder epilogue; every downstream grad is then zero via
            # the c>0 gating, so the rest of the pipeline is unchanged
            self.dict_sizes = b["dict_size"].detach().reshape(self.n_models).to(dev, torch.int32).contiguous()

        # per-feature lr multiplier for the post-resample warmup (Anthropic
        # protocol): the resampler writes ramp values in place, the Adam
        # kernels read it every step — allocated here (not in _alloc) so a
        # batch-size change never resets an active warmup, and hipGraph
        # capture sees a stable pointer
        self.lr_mult = torch.ones(self.n_models, self.n_dict, device=dev)

    def _alloc_workspaces(self, B: int):
        M, n, d = self.n_models, self.n_dict, self.d_act
        f = self._empty
        self.c = f(M, B, n)
        self.gpre = f(M, B, n)
        self.r = f(M, B, d)
        self.norms = f(M, n)
        self.inv_norms = f(M, n)
        self.loss_parts = f(M, 2)
        self.fired = self._zeros(M, n)  # accumulated across steps for resampling
        self.g_bias = f(M, n)
        self.gw = f(M, n, d)
        if self.kc["staging"] == "pre":
            # pre-transposed operands: every GEMM's staging direct/b128
            self.xT = f(d, B)
            self.rT = f(M, d, B)
            self.WT = f(M, d, n)
            if not self.tied:
                self.WencT = f(M, d, n)
        if not self.tied:
            self.gw_enc = f(M, n, d)

    def _grads(self, x, B, on_grads):
        p = self.ens.params
        bias = p["encoder_bias"]
        dict_w = p["encoder"] if self.tied else p["decoder"]
        self.loss_parts.zero_()
        if self.kc["staging"] != "pre":
            self._chain(x, dict_w, bias, enc_mode=3 if self.reverse else 0,
                        gc_mode=1 if self.reverse else 0, on_grads=on_grads)
            return

        # pre-transpose once per step so the big GEMMs stage all operands
        # directly (b128 LDS writes): x^T, What^T (inv-norm pre-applied)
        ext, bk, prio = self.ext, self.bk, self.prio
        self.g_bias.zero_()  # k_gc2 accumulates into it
        ext.row_norms(dict_w, self.norms, self.inv_norms, EPS_NORM)
        ext.transpose_scale(x, self.xT, None)
        ext.transpose_scale(dict_w, self.WT, self.inv_norms)
        WencT = self.WT
        if not self.tied:
            WencT = self.WencT
            ext.transpose_scale(p["encoder"], WencT, None)
        ext.enc_fwd2(self.xT, WencT, bias, self.c, self.loss_parts, self.fired, 0, bk, prio,
                     dict_sizes=self.dict_sizes)
        ext.dec_fwd(self.c, dict_w, self.inv_norms, x, self.r, self.loss_parts, self.bk_dec, prio)
        ext.transpose_scale(self.r, self.rT, None)
        ext.gc2(self.rT, self.WT, self.c, self.l1_alpha, self.gpre, self.g_bias, bk, prio)
        _announce(on_grads, self.g_bias)
        self._weight_grads(x, B, on_grads)

    def _chain(self, x, dict_w, bias, enc_mode=0, gc_mode=0, on_grads=None):
        """The transpose-in-staging launch chain (no separate transpose
        kernels): row norms -> enc_fwd -> dec_fwd -> gc -> weight grads.

        x is the input the pipeline sees, shared [B, d] or per-model
        [M, B, d]; dict_w the dictionary it runs on (the tied encoder, a
        clamped copy of it, or the untied decoder).  With on_grads the
        gradients are announced as they become final (g_bias after k_gc, the
        weight grads in chunks); without it the caller announces them."""
        ext, bk, prio = self.ext, self.bk, self.prio
        B = x.shape[-2]
        enc, enc_inv = (dict_w, self.inv_norms) if self.tied else (self.ens.params["encoder"], None)
        if gc_mode == 1:
            self.g_bias.zero_()  # the reverse k_gc writes no bias gradient
        ext.row_norms(dict_w, self.norms, self.inv_norms, EPS_NORM)
        ext.enc_fwd(x, enc, bias, enc_inv, self.c, self.loss_parts, self.fired, enc_mode, bk, prio,
                    self.bn_enc, dict_sizes=self.dict_sizes)
        ext.dec_fwd(self.c, dict_w, self.inv_norms, x, self.r, self.loss_parts, self.bk_dec, prio, self.bn)
        # gc_mode 0 overwrites g_bias (accumulate=False): no memset needed
        ext.gc(self.r, dict_w, self.inv_norms, self.c, self.l1_alpha, self.gpre, self.g_bias, bk, prio,
               gc_mode=gc_mode, bn=self.bn_enc, accumulate=False)
        _announce(on_grads, self.g_bias)  # final after k_gc
        self._weight_grads(x, B, on_grads)

    def _weight_grads(self, x, B, on_grads=None):
        """gw = gscale c^T r (+ gpre^T x when tied, else gw_enc = gpre^T x)."""
        ext, prio, bn, bk_gw = self.ext, self.prio, self.bn, self.bk_gw
        M = self.n_models
        gscale = 2.0 / (B * self.d_act)
        if self.tied and on_grads is not None and M > 1:
            # chunk the weight-grad GEMMs over model groups so each chunk's
            # all-reduce rides under the next chunk's compute; quarters keep
            # the exposed tail to one chunk's reduce (xGMI ring: ~2*S*7/8 /
            # 153 GB/s per link for an S-byte chunk)
            n_chunks = min(M, 4)
            bounds = [M * i // n_chunks for i in range(n_chunks + 1)]
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                sl = slice(lo, hi)
                ext.grad_w(self.c[sl], self.r[sl], self.gw[sl], gscale, 0.0, bk_gw, prio, bn)
                ext.grad_w(self.gpre[sl], x[sl] if x.dim() == 3 else x, self.gw[sl], 1.0, 1.0, bk_gw, prio, bn)
                on_grads([self.gw[sl]])
        elif self.tied:
            ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio, bn)
            ext.grad_w(self.gpre, x, self.gw, 1.0, 1.0, bk_gw, prio, bn)
            _announce(on_grads, self.gw)  # M == 1: single unchunked grad tensor
        else:
            ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio, bn)
            _announce(on_grads, self.gw)
            ext.grad_w(self.gpre, x, self.gw_enc, 1.0, 0.0, bk_gw, prio, bn)
            _announce(on_grads, self.gw_enc)

    def _matrix_updates(self):
        """(parameter key, gradient workspace, project) per matrix update."""
        if self.tied:
            return [("encoder", self.gw, True)]
        return [("decoder", self.gw, True), ("encoder", self.gw_enc, False)]

    def update_phase(self, B: int):
        """Adam updates (projection through the renorm for the dictionary)."""
        t = self._begin_update()
        for key, grad, project in self._matrix_updates():
            self._adam_matrix(key, grad, t, project=project, lr_mult=self.lr_mult)
        self._update_bias(t)

    def _update_bias(self, t):
        self._adam_vector("encoder_bias", self.g_bias, t, decay=self.bias_decay, lr_mult=self.lr_mult)

    # -- row-sharded update (data-parallel rs_ag) -----------------------------
    @property
    def row_shardable(self) -> bool:
        """Whether update_phase is the plain table above, so that a trainer
        may run it on row shards (_adam_matrix rows=) plus _update_bias."""
        return type(self) is HipSAEStep and not self.masked and not self.reverse

    def locate_grad(self, t: torch.Tensor):
        """The _matrix_updates entry whose gradient workspace holds t (a
        tensor handed to on_grads) and t's first row in its [M*n, d] view."""
        for entry in self._matrix_updates():
            g = entry[1]
            off = t.storage_offset() - g.storage_offset()
            if t.untyped_storage().data_ptr() == g.untyped_storage().data_ptr() and 0 <= off < g.numel():
                return entry, off // self.d_act
        raise RuntimeError("gradient tensor not in a known workspace")

    def _loss_data(self, B: int):
        out = self._mse_l1_loss(B, self.loss_parts[:, 1])
        if self.masked:  # masked losses carry no bias-decay term
            return out
        bias = self.ens.params["encoder_bias"]
        l_bd = self.bias_decay * torch.norm(bias, 2, dim=-1)
        out["loss"] = out["loss"] + l_bd
        out["l_bias_decay"] = l_bd
        return out

    def dp_grad_tensors(self):
        ts = [self.gw, self.g_bias]
        if not self.tied:
            ts.append(self.gw_enc)
        return ts


class HipCenteredStep(HipSAEStep):
    """Fused step for FunctionalTiedCenteredSAE (sae_ensemble.py:164-230):
    the tied pipeline runs on the per-model centered input x' = x - t[m]
    (enc/dec kernels take an [M,B,d] x with a model stride), and the
    learnable center's gradient falls out of workspaces that already exist:
        dL/dt = gscale * sum_b r_b  -  g_bias @ What
    (g_bias is the column sum of gpre from k_gc)."""

    staging = "t"  # the per-model-x-stride kernels live in the "t" path

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)

    def _alloc_workspaces(self, B: int):
        super()._alloc_workspaces(B)
        self.xc = self._empty(self.n_models, B, self.d_act)
        self.g_center = self._empty(self.n_models, self.d_act)

    def _grads(self, x, B, on_grads):
        p = self.ens.params
        enc = p["encoder"]
        self.loss_parts.zero_()
        torch.sub(x.unsqueeze(0), p["center"].unsqueeze(1), out=self.xc)
        self._chain(self.xc, enc, p["encoder_bias"])
        # center gradient from existing reductions (docstring derivation);
        # column sum via the coalesced k_colsum kernel
        self.ext.colsum(self.r, self.g_center, 2.0 / (B * self.d_act))
        self.g_center.sub_(torch.einsum("mn,mnd->md", self.g_bias * self.inv_norms, enc))
        _announce(on_grads, self.gw, self.g_bias, self.g_center)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("encoder", self.gw, t, project=True, lr_mult=self.lr_mult)
        self._adam_vector("encoder_bias", self.g_bias, t, lr_mult=self.lr_mult)
        self._adam_vector("center", self.g_center, t)

    def _loss_data(self, B: int):
        return self._mse_l1_loss(B, self.loss_parts[:, 1])

    def dp_grad_tensors(self):
        return [self.gw, self.g_bias, self.g_center]


class HipWhitenedStep(HipSAEStep):
    """Fused step for FunctionalTiedSAE with GENERAL affine
    whitening-centering buffers (K7; reference sae_ensemble.py:98-132,
    :127-132 center / :148 loss-in-centered-space).

    The buffers are non-trainable, and the loss lives entirely in the
    centered space x' = ((x - t[m]) @ rot[m]^T) * s[m], so the step is the
    plain tied pipeline on a per-model centered input ([M, B, d], same
    model-stride kernels as HipCenteredStep) after ONE batched [d, d] GEMM:
    x' = (x - t) @ Wc with Wc = (rot * s[:, None])^T precomputed."""

    staging = "t"  # the per-model-x-stride kernels live in the "t" path

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)
        b = ensemble.buffers
        rot = b["center_rot"].detach().float()
        scale = b["center_scale"].detach().float()
        self.trans = b["center_trans"].detach().float().contiguous()
        # result[b, c] = sum_u (x-t)[b, u] * rot[c, u] * s[c]
        self.Wc = (rot * scale.unsqueeze(-1)).transpose(1, 2).contiguous()  # [M, d, d]

    def _alloc_workspaces(self, B: int):
        super()._alloc_workspaces(B)
        self.xsub = self._empty(self.n_models, B, self.d_act)
        self.xc = self._empty(self.n_models, B, self.d_act)

    def _grads(self, x, B, on_grads):
        p = self.ens.params
        self.loss_parts.zero_()
        torch.sub(x.unsqueeze(0), self.trans.unsqueeze(1), out=self.xsub)
        torch.bmm(self.xsub, self.Wc, out=self.xc)  # library GEMM: plain batched matmul
        self._chain(self.xc, p["encoder"], p["encoder_bias"])
        _announce(on_grads, self.gw, self.g_bias)
    # update_phase / _loss_data: inherited tied versions (incl. bias decay)


class HipPositiveStep(HipSAEStep):
    """Fused step for FunctionalPositiveTiedSAE (mlp_tests.py:68-125):
    the tied pipeline runs on Wc = clamp(W, 0) and the shifted input
    x' = x + 0.18; the projected gradient is masked by the clamp derivative
    before Adam updates the raw (signed) encoder."""

    staging = "t"

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)

    def _alloc_workspaces(self, B: int):
        super()._alloc_workspaces(B)
        self.Wc = self._empty(self.n_models, self.n_dict, self.d_act)
        self.x_shift = self._empty(B, self.d_act)

    def _grads(self, x, B, on_grads):
        from sparse_coding_amd.models.positive import INPUT_SHIFT

        p = self.ens.params
        self.loss_parts.zero_()
        torch.clamp(p["encoder"], min=0.0, out=self.Wc)
        torch.add(x, INPUT_SHIFT, out=self.x_shift)
        self._chain(self.x_shift, self.Wc, p["encoder_bias"])
        _announce(on_grads, self.gw, self.g_bias)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("encoder", self.gw, t, project=True, lr_mult=self.lr_mult,
                          w_used=self.Wc, clamp_mask=True)
        self._adam_vector("encoder_bias", self.g_bias, t, decay=self.bias_decay, lr_mult=self.lr_mult)


class HipThresholdStep(HipSAEStep):
    """Fused step for FunctionalThresholdingSAE.

    Tied dictionary with a learned soft-threshold gate instead of bias+ReLU
    (reference sae_ensemble.py:232-289): the encoder GEMM runs with a gate
    epilogue (k_enc_fwd_t mode 2) that keeps u = (c+gain)/max(a^2,eps) for
    the backward, and k_gc_thresh_t pushes dL/dcode through g'(u) while
    accumulating the per-feature gain/scale gradients as column sums.
    Weight grads + renorm-projected Adam are the tied-SAE kernels.
    """

    staging = "t"  # the gate epilogue lives only in the transpose-in-staging kernels

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)

    def _alloc_workspaces(self, B: int):
        super()._alloc_workspaces(B)
        M, n = self.n_models, self.n_dict
        self.u = self._empty(M, B, n)
        self.g_gain = self._zeros(M, n)
        self.g_scale = self._zeros(M, n)
        self.dummy_bias = self._zeros(M, n)

    def _grads(self, x, B, on_grads):
        ext, bk, prio = self.ext, self.bk, self.prio
        p = self.ens.params
        enc = p["encoder"]
        a = p["activation_scale"]

        self.loss_parts.zero_()
        self.g_gain.zero_()
        self.g_scale.zero_()

        ext.row_norms(enc, self.norms, self.inv_norms, EPS_NORM)
        ext.enc_fwd(x, enc, self.dummy_bias, self.inv_norms, self.c, self.loss_parts, self.fired, 2,
                    bk, prio, self.bn_enc, act_scale=a, act_gain=p["activation_gain"], u_out=self.u)
        ext.dec_fwd(self.c, enc, self.inv_norms, x, self.r, self.loss_parts, self.bk_dec, prio, self.bn)
        ext.gc_thresh(self.r, enc, self.inv_norms, self.c, self.u, a,
                      self.l1_alpha, self.gpre, self.g_gain, self.g_scale, bk, prio)
        self._weight_grads(x, B)
        _announce(on_grads, self.gw, self.g_gain, self.g_scale)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("encoder", self.gw, t, project=True, lr_mult=self.lr_mult)
        self._adam_vector("activation_scale", self.g_scale, t, lr_mult=self.lr_mult)
        self._adam_vector("activation_gain", self.g_gain, t, lr_mult=self.lr_mult)

    def _loss_data(self, B: int):
        return self._mse_l1_loss(B, self.loss_parts[:, 1])

    def dp_grad_tensors(self):
        return [self.gw, self.g_gain, self.g_scale]


class HipLISTAStep(_HipStep):
    """Fused training step for FunctionalLISTADenoisingSAE (SURVEY.md K11;
    reference residual_denoising_autoencoder.py:15-122).

    Every GEMM runs on the MFMA kernels, and ALL the elementwise work is
    fused into them or into one custom pass:
      * forward: k_enc_fwd mode 4 computes r = y - (neg_e W_l^T),
        x = shrink(r, theta) and y' = x + m (x - x_prev) in the GEMM
        epilogue (one kernel per layer after the neg_e product);
      * backward: k_lista_bwd_elem replaces the g_x/g_r/g_theta/g_rho
        elementwise chain with one coalesced pass; k_enc_fwd mode 5 writes
        g_y = g_r - g_e A_hat^T straight out of the GEMM.
    The whole step is hipGraph-captured like the plain SAE step.

    Backward, per layer (hand-derived, oracle-tested):
      g_x = (1+m) g_y + carry;  g_r = g_x [|r| > theta]
      g_theta = -sum_b g_r sign(r);  g_rho = sum g_y (x - x_prev) [0<rho<1]
      g_W = -g_r^T neg_e;  g_e = g_r W_l;  g_y_prev = g_r - g_e A_hat^T
      carry' = -m g_y;  g_Ahat -= y_prev^T g_e
    plus g_Ahat += gscale c^T rr + g_y0^T b, projected by k_project_adam.
    """

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext)
        self.n_layers = len(ensemble.params["encoder_layers"])
        # rho's Adam runs as torch ops.  The Adam kernels receive the betas as
        # fp32 and form 1 - beta exactly; the same two values here, so that
        # every parameter of the step runs one recurrence (1 - 0.999 rounded to
        # fp32 on its own is 4.7e-5 off 1 - fp32(0.999), which the bias
        # correction 1 - beta^t does not undo)
        self._b1, self._b2 = (torch.tensor(b, dtype=torch.float32).item() for b in (self.beta1, self.beta2))

    @property
    def codes(self):
        return self.y[self.n_layers]

    def _alloc_workspaces(self, B: int):
        M, n, d, L = self.n_models, self.n_dict, self.d_act, self.n_layers
        f = self._empty
        self.norms, self.inv_norms = f(M, n), f(M, n)
        self.ones_mn = self._ones(M, n)
        self.zeros_bd = self._zeros(B, d)
        self.scratch_lp = f(M, 2)
        self.loss_parts = f(M, 2)
        self.fired = self._zeros(M, n)
        self.mom = [f(M) for _ in range(L)]
        # forward saves
        self.y = [f(M, B, n) for _ in range(L + 1)]
        self.x = [f(M, B, n) for _ in range(L + 1)]
        self.r = [f(M, B, n) for _ in range(L)]
        self.neg_e = [f(M, B, d) for _ in range(L)]
        self.rr = f(M, B, d)
        # backward workspaces
        self.g_y = f(M, B, n)
        self.g_r = f(M, B, n)
        self.carry_a = self._zeros(M, B, n)
        self.carry_b = self._zeros(M, B, n)
        self.sgn = f(M, B, n)
        self.g_e = f(M, B, d)
        self.gA = f(M, n, d)
        self.gW = [f(M, n, d) for _ in range(L)]
        self.g_theta = [f(M, n) for _ in range(L)]
        self.g_rho = [f(M) for _ in range(L)]
        self.scratch_mn = f(M, n)

    def _grads(self, b, B, on_grads):
        ext = self.ext
        M, d, L = self.n_models, self.d_act, self.n_layers
        p = self.ens.params
        A = p["decoder"]
        layers = p["encoder_layers"]
        bk, prio, bk_dec, bk_gw = self.bk, self.prio, self.bk_dec, self.bk_gw

        self.loss_parts.zero_()
        ext.row_norms(A, self.norms, self.inv_norms, EPS_NORM)

        # ---- forward ----
        ext.enc_fwd(b, A, self.ones_mn, self.inv_norms, self.y[0],
                    self.scratch_lp, self.fired, 1, bk, prio)
        self.x[0].copy_(self.y[0])
        for l in range(L):
            torch.clamp(layers[l]["rho"].reshape(M), 0.0, 1.0, out=self.mom[l])
            ext.dec_fwd(self.y[l], A, self.inv_norms, b, self.neg_e[l],
                        self.scratch_lp, bk_dec, prio)
            # GEMM (neg_e W_l^T) + fused shrink/momentum epilogue
            ext.enc_fwd(self.neg_e[l], layers[l]["W"], self.ones_mn, None,
                        self.y[l + 1], self.scratch_lp, self.fired, 4, bk, prio,
                        act_scale=layers[l]["theta"], u_out=self.r[l],
                        y_in=self.y[l], x_prev=self.x[l], x_out=self.x[l + 1],
                        mom=self.mom[l])
        c = self.y[L]
        ext.dec_fwd(c, A, self.inv_norms, b, self.rr, self.loss_parts, bk_dec, prio)

        # ---- backward ----
        gscale = 2.0 / (B * d)
        ext.enc_fwd(self.rr, A, self.ones_mn, self.inv_norms, self.g_y,
                    self.scratch_lp, self.fired, 1, bk, prio)
        self.g_y.mul_(gscale)
        torch.sign(c, out=self.sgn)
        self.sgn.mul_((self.l1_alpha / B).reshape(M, 1, 1))
        self.g_y.add_(self.sgn)
        ext.grad_w(c, self.rr, self.gA, gscale, 0.0, bk_gw, prio)

        carry_in, carry_out = None, self.carry_a
        for l in range(L - 1, -1, -1):
            self.g_theta[l].zero_()
            self.g_rho[l].zero_()
            ext.lista_bwd_elem(self.g_y, carry_in, self.r[l], layers[l]["theta"],
                               self.x[l + 1], self.x[l], self.mom[l],
                               self.g_r, carry_out, self.g_theta[l], self.g_rho[l])
            ext.grad_w(self.g_r, self.neg_e[l], self.gW[l], -1.0, 0.0, bk_gw, prio)
            _announce(on_grads, self.gW[l], self.g_theta[l], self.g_rho[l])
            ext.dec_fwd(self.g_r, layers[l]["W"], self.ones_mn, self.zeros_bd,
                        self.g_e, self.scratch_lp, bk_dec, prio)
            ext.grad_w(self.y[l], self.g_e, self.gA, -1.0, 1.0, bk_gw, prio)
            # g_y_prev = g_r - g_e A_hat^T (mode-5 epilogue)
            ext.enc_fwd(self.g_e, A, self.ones_mn, self.inv_norms, self.g_y,
                        self.scratch_lp, self.fired, 5, bk, prio, y_in=self.g_r)
            carry_in = carry_out
            carry_out = self.carry_b if carry_in is self.carry_a else self.carry_a

        # x0 = y0: remaining carry lands on g_y0
        self.g_y.add_(carry_in)
        ext.grad_w(self.g_y, b, self.gA, 1.0, 1.0, bk_gw, prio)
        _announce(on_grads, self.gA)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("decoder", self.gA, t, project=True)
        for l in range(self.n_layers):
            self._adam_matrix(("encoder_layers", l, "W"), self.gW[l], t, project=False)
            self._adam_vector(("encoder_layers", l, "theta"), self.g_theta[l], t)
            # clamp gate on rho (identical on every DP rank)
            rho = self.ens.params["encoder_layers"][l]["rho"].reshape(self.n_models)
            self.g_rho[l].mul_(((rho > 0.0) & (rho < 1.0)).float())
            self._apply_rho_adam(l, t)

    def _apply_rho_adam(self, l, step_no):
        rho, mu, nu = self._param_state(("encoder_layers", l, "rho"))
        g = self.g_rho[l].reshape(rho.shape)
        t = step_no.reshape(rho.shape)
        b1, b2 = self._b1, self._b2
        mu.mul_(b1).add_(g, alpha=1 - b1)
        nu.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = 1 - torch.pow(b1, t)
        bc2 = 1 - torch.pow(b2, t)
        rho.sub_(self.lr * (mu / bc1) / ((nu / bc2).sqrt() + self.eps))

    def _loss_data(self, B: int):
        self.ext.colsum(self.codes, self.scratch_mn, absval=True)
        return self._mse_l1_loss(B, self.scratch_mn.sum(dim=1))

    def dp_grad_tensors(self):
        return [self.gA] + self.gW + self.g_theta + self.g_rho


class HipResidualDenoisingStep(_HipStep):
    """Fused step for FunctionalResidualDenoisingSAE
    (residual_denoising_autoencoder.py:125-201): x0 = b A_hat^T, then
    L residual blocks x' = relu(x + theta_l) W_l^T + x (W_l is [n, n]),
    c = relu(x_L + bias).  Same kernel-orchestration recipe as HipLISTAStep;
    all GEMMs (including the [n,n] layer products) run on the MFMA kernels.
    """

    # runs eagerly: turning capture on is a performance change, to be measured on its own
    captures_graph = False

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext)
        self.n_layers = len(ensemble.params["encoder_layers"])

    def _alloc_workspaces(self, B: int):
        M, n, d, L = self.n_models, self.n_dict, self.d_act, self.n_layers
        f = self._empty
        self.norms, self.inv_norms = f(M, n), f(M, n)
        self.ones_mn = self._ones(M, n)
        self.zeros_bn = self._zeros(B, n)
        self.scratch_lp = f(M, 2)
        self.loss_parts = f(M, 2)
        self.fired = self._zeros(M, n)
        self.xs = [f(M, B, n) for _ in range(L + 1)]
        self.hs = [f(M, B, n) for _ in range(L)]
        self.c = f(M, B, n)
        self.rr = f(M, B, d)
        self.g_x = f(M, B, n)
        self.g_h = f(M, B, n)
        self.gA = f(M, n, d)
        self.gW = [f(M, n, n) for _ in range(L)]
        self.g_theta = [f(M, n) for _ in range(L)]
        self.g_bias = f(M, n)
        self.scratch_mn = f(M, n)

    def _grads(self, b, B, on_grads):
        ext = self.ext
        L = self.n_layers
        p = self.ens.params
        A = p["decoder"]
        layers = p["encoder_layers"]
        bk, prio, bk_dec, bk_gw = self.bk, self.prio, self.bk_dec, self.bk_gw

        self.loss_parts.zero_()
        ext.row_norms(A, self.norms, self.inv_norms, EPS_NORM)

        # forward
        ext.enc_fwd(b, A, self.ones_mn, self.inv_norms, self.xs[0],
                    self.scratch_lp, self.fired, 1, bk, prio)
        for l in range(L):
            W_l, theta = layers[l]["W"], layers[l]["theta"]
            torch.add(self.xs[l], theta.unsqueeze(1), out=self.hs[l])
            self.hs[l].clamp_(min=0.0)
            # x' = h W_l^T + x  ([M,B,n] x [M,n,n])
            ext.enc_fwd(self.hs[l], W_l, self.ones_mn, None, self.xs[l + 1],
                        self.scratch_lp, self.fired, 1, bk, prio)
            self.xs[l + 1].add_(self.xs[l])
        torch.add(self.xs[L], p["encoder_bias"].unsqueeze(1), out=self.c)
        self.c.clamp_(min=0.0)

        ext.dec_fwd(self.c, A, self.inv_norms, b, self.rr, self.loss_parts, bk_dec, prio)
        # c >= 0, so the L1 sum is a column sum + tiny [M, n] reduce; the
        # torch sum(dim=(1,2)) dispatched a 1.79 ms strided reduce
        # (profiles/r02_residual_kernel_stats.csv)
        ext.colsum(self.c, self.scratch_mn)
        self._l1_sum = self.scratch_mn.sum(dim=1)

        # backward: g_c via k_gc (relu mask + l1 term + bias colsum, K=d)
        ext.gc(self.rr, A, self.inv_norms, self.c, self.l1_alpha,
               self.g_x, self.g_bias, bk, prio, accumulate=False)
        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.rr, self.gA, gscale, 0.0, bk_gw, prio)

        for l in range(L - 1, -1, -1):
            # g_W_l = g_x'^T h
            ext.grad_w(self.g_x, self.hs[l], self.gW[l], 1.0, 0.0, bk_gw, prio)
            _announce(on_grads, self.gW[l])
            # g_h = g_x' @ W_l  ([M,B,n] x [M,n,n])
            ext.dec_fwd(self.g_x, layers[l]["W"], self.ones_mn, self.zeros_bn, self.g_h,
                        self.scratch_lp, bk_dec, prio)
            # relu(x + theta) backward
            self.g_h.mul_((self.hs[l] > 0).float())
            # column sum via k_colsum: torch.sum(dim=1) dispatches a strided
            # reduce at ~140 GB/s (rocprof r02_residual_kernel_stats: 1.79 ms
            # = 5% of the step); the coalesced-row kernel streams the same
            # bytes at HBM rate
            ext.colsum(self.g_h, self.g_theta[l])
            _announce(on_grads, self.g_theta[l])
            self.g_x.add_(self.g_h)  # residual skip + through-layer paths

        # x0 = b A_hat^T
        ext.grad_w(self.g_x, b, self.gA, 1.0, 1.0, bk_gw, prio)
        _announce(on_grads, self.gA, self.g_bias)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("decoder", self.gA, t, project=True)
        for l in range(self.n_layers):
            self._adam_matrix(("encoder_layers", l, "W"), self.gW[l], t, project=False)
            self._adam_vector(("encoder_layers", l, "theta"), self.g_theta[l], t)
        self._adam_vector("encoder_bias", self.g_bias, t)

    def _loss_data(self, B: int):
        return self._mse_l1_loss(B, self._l1_sum)

    def dp_grad_tensors(self):
        return [self.gA, self.g_bias] + self.gW + self.g_theta


class HipSemilinearStep(_HipStep):
    """Fused step for SemiLinearSAE (semilinear_autoencoder.py:14-83): a
    2-layer relu MLP encoder + normalized linear decoder.  The top-layer
    backward IS k_gc (relu mask + l1 + bias column sums); the hidden layer
    is one more GEMM pair.
    """

    # runs eagerly: turning capture on is a performance change, to be measured on its own
    captures_graph = False

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext)
        layers = ensemble.params["encoder_layers"]
        assert len(layers) == 2
        self.hidden = layers[0]["weight"].shape[1]  # [M, h, d] -> h

    def _alloc_workspaces(self, B: int):
        M, n, d, h = self.n_models, self.n_dict, self.d_act, self.hidden
        f = self._empty
        self.norms, self.inv_norms = f(M, n), f(M, n)
        # unit row scales for the g_c W2 product: one per row of W2 [M, n, h]
        self.ones_mn = self._ones(M, n)
        self.zeros_bh = self._zeros(B, h)
        self.scratch_lp = f(M, 2)
        self.loss_parts = f(M, 2)
        self.fired = self._zeros(M, n)
        self.fired_h = self._zeros(M, h)
        self.h1 = f(M, B, h)
        self.c = f(M, B, n)
        self.rr = f(M, B, d)
        self.g_c = f(M, B, n)
        self.g_h = f(M, B, h)
        self.gA = f(M, n, d)
        self.gW2 = f(M, n, h)
        self.gW1 = f(M, h, d)
        self.g_b2 = f(M, n)
        self.g_b1 = f(M, h)
        self.scratch_mn = f(M, n)

    def _grads(self, b, B, on_grads):
        ext = self.ext
        p = self.ens.params
        A = p["decoder"]
        l1p, l2p = p["encoder_layers"]
        bk, prio, bk_dec, bk_gw = self.bk, self.prio, self.bk_dec, self.bk_gw

        self.loss_parts.zero_()
        ext.row_norms(A, self.norms, self.inv_norms, EPS_NORM)

        # h1 = relu(b W1^T + b1);  c = relu(h1 W2^T + b2)
        ext.enc_fwd(b, l1p["weight"], l1p["bias"], None, self.h1,
                    self.scratch_lp, self.fired_h, 0, bk, prio)
        ext.enc_fwd(self.h1, l2p["weight"], l2p["bias"], None, self.c,
                    self.scratch_lp, self.fired, 0, bk, prio)
        ext.dec_fwd(self.c, A, self.inv_norms, b, self.rr, self.loss_parts, bk_dec, prio)
        # c >= 0: L1 via the coalesced column-sum kernel (the torch
        # sum(dim=(1,2)) was 9%% of this step)
        ext.colsum(self.c, self.scratch_mn)
        self._l1_sum = self.scratch_mn.sum(dim=1)

        # backward
        ext.gc(self.rr, A, self.inv_norms, self.c, self.l1_alpha,
               self.g_c, self.g_b2, bk, prio, accumulate=False)
        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.rr, self.gA, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.g_c, self.h1, self.gW2, 1.0, 0.0, bk_gw, prio)
        # g_h1 = (g_c W2) * [h1 > 0]
        ext.dec_fwd(self.g_c, l2p["weight"], self.ones_mn, self.zeros_bh,
                    self.g_h, self.scratch_lp, bk_dec, prio)
        self.g_h.mul_((self.h1 > 0).float())
        # strided-reduce -> k_colsum (9% of the semilinear step,
        # rocprof r02_semilinear_kernel_stats)
        ext.colsum(self.g_h, self.g_b1)
        ext.grad_w(self.g_h, b, self.gW1, 1.0, 0.0, bk_gw, prio)
        _announce(on_grads, self.gA, self.gW2, self.gW1, self.g_b2, self.g_b1)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("decoder", self.gA, t, project=True)
        for li, (gW, gb) in enumerate(((self.gW1, self.g_b1), (self.gW2, self.g_b2))):
            self._adam_matrix(("encoder_layers", li, "weight"), gW, t, project=False,
                              n_per_model=gW.shape[1])
            self._adam_vector(("encoder_layers", li, "bias"), gb, t)

    def _loss_data(self, B: int):
        return self._mse_l1_loss(B, self._l1_sum)

    def dp_grad_tensors(self):
        return [self.gA, self.gW1, self.gW2, self.g_b1, self.g_b2]


class HipTopKStep(_HipStep):
    """Fused TopK-encoder training step.

    Same GEMM pipeline as the tied SAE but: raw-score encoder (no bias/relu),
    per-row top-k selection + scatter + relu between encode and decode, no L1
    term, and the dictionary normalization has NO eps clamp
    (reference topk_encoder.py:31).  The per-model k lives in
    buffers["sparsity"]; selection runs in one kernel (k_topk_select).
    """

    EPS = 1e-30  # un-clamped normalization (reference divides by the raw norm)
    dict_key = "dict"

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext)
        dev = self._dev
        self.ks = [int(k) for k in ensemble.buffers["sparsity"].reshape(-1).tolist()]
        self.ks_i32 = torch.tensor(self.ks, device=dev, dtype=torch.int32)
        self.zero_l1 = torch.zeros(self.n_models, device=dev)
        self.dummy_bias = torch.zeros(self.n_models, self.n_dict, device=dev)
        self.lr_mult = torch.ones(self.n_models, self.n_dict, device=dev)

    def _alloc_workspaces(self, B: int):
        M, n, d = self.n_models, self.n_dict, self.d_act
        f = self._empty
        self.scores = f(M, B, n)
        self.c = f(M, B, n)
        self.gpre = f(M, B, n)
        self.r = f(M, B, d)
        self.norms = f(M, n)
        self.inv_norms = f(M, n)
        self.loss_parts = f(M, 2)
        self.fired = self._zeros(M, n)
        self.g_bias_scratch = f(M, n)
        self.gw = f(M, n, d)

    def _grads(self, x, B, on_grads):
        ext, bk, prio, bk_gw = self.ext, self.bk, self.prio, self.bk_gw
        W = self.ens.params["dict"]

        self.loss_parts.zero_()
        ext.row_norms(W, self.norms, self.inv_norms, self.EPS)
        ext.enc_fwd(x, W, self.dummy_bias, self.inv_norms,
                    self.scores, self.loss_parts, self.fired, 1, bk, prio)
        self._select()

        ext.dec_fwd(self.c, W, self.inv_norms, x, self.r, self.loss_parts, self.bk_dec, prio)
        ext.gc(self.r, W, self.inv_norms, self.c, self.zero_l1,
               self.gpre, self.g_bias_scratch, bk, prio, accumulate=False)
        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.gpre, x, self.gw, 1.0, 1.0, bk_gw, prio)
        _announce(on_grads, self.gw)

    def _select(self):
        """scores -> codes c (+ fired counts)."""
        # exact per-row radix top-k + scatter + fired counts in ONE kernel
        # (k_topk_select) — replaces the torch.topk/scatter chain
        self.ext.topk_select(self.scores, self.c, self.fired, self.ks_i32)

    def update_phase(self, B: int):
        t = self._begin_update()
        self._adam_matrix("dict", self.gw, t, project=True, lr_mult=self.lr_mult, eps_norm=self.EPS)

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        return {"loss": mse}

    def dp_grad_tensors(self):
        return [self.gw]


class HipBatchTopKStep(HipTopKStep):
    """Fused BatchTopK training step: the TopK chain with the per-row
    selection replaced by a batch-level one (models/batch_topk.py).

    Per model the K = min(k*B, B*n) largest of all B*n scores are kept, ties
    at the K-th value included.  The selection is an exact multi-workgroup
    radix select (k_btk_hist x3 + k_btk_write behind ext.batch_topk_select):
    no host read, K computed on the device, captured in the step's hipGraph
    with the rest of the chain.  The write pass also reports the batch's
    selection threshold (``thr_batch``, returned as loss_data["threshold"])
    and folds it into the inference-threshold state.

    That state (buffers "threshold", "threshold_n", "threshold_lr") is read
    from ``ens.buffers`` at every launch, not at construction: a resumed
    sweep replaces the whole buffer tree.  A captured graph holds the
    buffers' addresses, so when they change the graph is dropped and
    captured again.

    Under data parallelism each rank selects on its local batch and keeps
    its own threshold state; the thresholds are not synchronised across
    ranks.
    """

    _STATE = ("threshold", "threshold_n", "threshold_lr")

    def _alloc_workspaces(self, B: int):
        super()._alloc_workspaces(B)
        M = self.n_models
        self.thr_batch = self._empty(M)
        self.btk_work = torch.empty(self.ext.batch_topk_workspace_size(M), device=self._dev,
                                    dtype=torch.int32)

    def _state_ptrs(self):
        return tuple(self.ens.buffers[k].data_ptr() for k in self._STATE)

    def _select(self):
        b = self.ens.buffers
        self.ext.batch_topk_select(self.scores, self.c, self.fired, self.ks_i32,
                                   self.thr_batch, self.btk_work,
                                   threshold=b["threshold"], threshold_n=b["threshold_n"],
                                   threshold_lr=b["threshold_lr"])

    def graph_key(self):
        return super().graph_key() + self._state_ptrs()

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        return {"loss": mse, "threshold": self.thr_batch}
