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

Fused-step coverage: EVERY trainable signature in the zoo — tied, untied,
masked tied/untied, thresholding, reverse, tied-centered, positive-tied,
TopK, LISTA, residual-denoising and semilinear.  The unrolled/MLP encoders
(HipLISTAStep / HipResidualDenoisingStep / HipSemilinearStep) orchestrate
the same MFMA GEMM kernels with hand-derived backward chains; elementwise
glue runs as torch ops on persistent workspaces.

All GEMMs run on the exact-f32 MFMA path (v_mfma_f32_32x32x2_f32): fp32 end
to end, the reference's training dtype.  Validated against the
torch/vmap oracle in tests/test_hip_numerics.py.

For multi-GPU DP the step splits at the gradient boundary
(`grads_phase` / `update_phase`) so the RCCL all-reduce of [M,n,d] grads
overlaps with nothing locally but lands between grad GEMMs and Adam.
"""

from __future__ import annotations

from typing import Optional

import torch

from sparse_coding_amd import ops as _ops
from sparse_coding_amd.models import sae_signatures as sigs

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


def maybe_make_step(ensemble, required: bool = False) -> Optional["HipSAEStep"]:
    """Return a HipSAEStep if (sig, device, buffers) are supported.

    On a CUDA device with a supported signature, a missing extension is a
    hard error: GPU runs must not silently fall back to eager."""
    import os

    if os.environ.get("SPARSE_CODING_AMD_FORCE_TORCH") == "1":
        return None

    dev = torch.device(ensemble.device) if not isinstance(ensemble.device, torch.device) else ensemble.device
    if dev.type != "cuda":
        if required:
            raise RuntimeError(f"backend='hip' requested but ensemble device is {dev}")
        return None

    sig = ensemble.sig
    from sparse_coding_amd.models.topk import TopKEncoder

    if sig is TopKEncoder:
        ext = _ops.get_extension(required=True)
        return HipTopKStep(ensemble, ext)

    if sig is sigs.FunctionalThresholdingSAE:
        ext = _ops.get_extension(required=True)
        return HipThresholdStep(ensemble, ext)

    if sig is sigs.FunctionalReverseSAE:
        ext = _ops.get_extension(required=True)
        return HipSAEStep(ensemble, ext, tied=True, reverse=True)

    if sig is sigs.FunctionalTiedCenteredSAE:
        ext = _ops.get_extension(required=True)
        return HipCenteredStep(ensemble, ext)

    from sparse_coding_amd.models.positive import FunctionalPositiveTiedSAE

    if sig is FunctionalPositiveTiedSAE:
        ext = _ops.get_extension(required=True)
        return HipPositiveStep(ensemble, ext)

    from sparse_coding_amd.models.lista import (
        FunctionalLISTADenoisingSAE,
        FunctionalResidualDenoisingSAE,
    )
    from sparse_coding_amd.models.semilinear import SemiLinearSAE

    if sig is FunctionalLISTADenoisingSAE:
        ext = _ops.get_extension(required=True)
        return HipLISTAStep(ensemble, ext)
    if sig is FunctionalResidualDenoisingSAE:
        ext = _ops.get_extension(required=True)
        return HipResidualDenoisingStep(ensemble, ext)
    if sig is SemiLinearSAE:
        ext = _ops.get_extension(required=True)
        return HipSemilinearStep(ensemble, ext)

    if sig is sigs.FunctionalMaskedTiedSAE:
        ext = _ops.get_extension(required=True)
        return HipSAEStep(ensemble, ext, tied=True, masked=True)
    if sig is sigs.FunctionalMaskedSAE:
        ext = _ops.get_extension(required=True)
        return HipSAEStep(ensemble, ext, tied=False, masked=True)

    tied = sig is sigs.FunctionalTiedSAE
    untied = sig is sigs.FunctionalSAE
    if not (tied or untied):
        if required:
            raise RuntimeError(f"backend='hip' requested but signature {sig.__name__} has no fused step yet")
        return None
    if tied and not _identity_centering(ensemble.buffers):
        # general affine whitening-centering (K7): PCA-whitened-input tied
        # SAE (reference sae_ensemble.py:98-132) — tied pipeline on a
        # precomputed per-model whitened input
        ext = _ops.get_extension(required=True)
        return HipWhitenedStep(ensemble, ext)

    ext = _ops.get_extension(required=True)  # loud on GPU
    return HipSAEStep(ensemble, ext, tied=tied)


class HipSAEStep:
    """Workspaces + kernel-sequence launcher for one ensemble."""

    def __init__(self, ensemble, ext, tied: bool, masked: bool = False, reverse: bool = False):
        self.ens = ensemble
        self.ext = ext
        self.tied = tied
        self.masked = masked
        # reverse SAE (sae_ensemble.py:447-503): code = pre * [pre+b > 0],
        # |code| in the L1, sign-aware backward, NO bias gradient from the
        # code path (only the L2-decay term moves the bias)
        self.reverse = reverse

        p = ensemble.params
        self.n_models, self.n_dict, self.d_act = p["encoder"].shape
        if not tied:
            assert p["decoder"].shape == p["encoder"].shape

        dev = p["encoder"].device
        b = ensemble.buffers
        self.l1_alpha = b["l1_alpha"].detach().to(dev, torch.float32).reshape(self.n_models).contiguous()
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

        opt = ensemble.optimizer_kwargs
        self.lr = float(opt.get("lr", 1e-3))
        betas = opt.get("betas", (0.9, 0.999))
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.eps = float(opt.get("eps", 1e-8))
        name = getattr(ensemble.optimizer_func, "__name__", "adam")
        if name != "adam":
            raise RuntimeError(f"fused HIP step supports adam only, got {name}")

        # per-feature lr multiplier for the post-resample warmup (Anthropic
        # protocol): the resampler writes ramp values in place, the Adam
        # kernels read it every step — allocated here (not in _alloc) so a
        # batch-size change never resets an active warmup, and hipGraph
        # capture sees a stable pointer
        self.lr_mult = torch.ones(self.n_models, self.n_dict, device=dev)

        # persistent workspaces, sized lazily on first batch
        self._B = None
        # hipGraph capture of the whole step (single-GPU path): replayed
        # after 2 eager warmup steps; disabled via SPARSE_CODING_AMD_NO_GRAPH=1
        import os as _os

        self.use_graph = _os.environ.get("SPARSE_CODING_AMD_NO_GRAPH") != "1"
        self._graph = None
        self._eager_steps = 0

    # -- workspace management -------------------------------------------------
    def _alloc(self, B: int):
        from sparse_coding_amd.ops.kconfig import kernel_config

        self.kc = kernel_config()
        M, n, d = self.n_models, self.n_dict, self.d_act
        dev = self.ens.params["encoder"].device
        f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        self.c = f(M, B, n)
        self.gpre = f(M, B, n)
        self.r = f(M, B, d)
        self.norms = f(M, n)
        self.inv_norms = f(M, n)
        self.loss_parts = f(M, 2)
        self.fired = torch.zeros(M, n, device=dev)
        self.g_bias = f(M, n)
        self.gw = f(M, n, d)
        if self.reverse:
            self.kc["staging"] = "t"
        if self.kc["staging"] == "pre":
            # pre-transposed operands: every GEMM's staging direct/b128
            self.xT = f(d, B)
            self.rT = f(M, d, B)
            self.WT = f(M, d, n)
            if not self.tied:
                self.WencT = f(M, d, n)
        if not self.tied:
            self.gw_enc = f(M, n, d)
        self._B = B
        self._graph = None
        self._eager_steps = 0

    # -- phases ---------------------------------------------------------------
    def grads_phase(self, x: torch.Tensor, on_grads=None):
        """Forward + backward: fills self.gw (+gw_enc), g_bias, loss parts.

        on_grads: optional callback(list_of_tensors) fired as gradient
        tensors become final — used by the DP trainer to launch RCCL
        all-reduces that overlap the remaining grad GEMMs (the [M,n,d]
        weight grads are chunked over model halves for this).
        """
        ens, ext = self.ens, self.ext
        M, n, d = self.n_models, self.n_dict, self.d_act
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)

        x = x.contiguous()
        p = ens.params
        enc = p["encoder"]
        bias = p["encoder_bias"]
        dict_w = enc if self.tied else p["decoder"]

        self.loss_parts.zero_()
        if self.reverse or self.kc["staging"] == "pre":
            self.g_bias.zero_()  # else k_gc overwrites it (accumulate=False)
        self._fired_step = self.fired  # accumulated across steps for resampling

        kc = self.kc
        bk, prio = kc["bk"], kc["prio"]
        bn = kc.get("bn", 128)
        bn_enc = kc.get("bn_enc") or bn
        bk_dec = kc["bk_dec"] or bk
        bk_gw = kc["bk_grad_w"] or bk

        ext.row_norms(dict_w, self.norms, self.inv_norms, EPS_NORM)
        if kc["staging"] == "pre":
            # pre-transpose once per step so the big GEMMs stage all operands
            # directly (b128 LDS writes): x^T, What^T (inv-norm pre-applied)
            ext.transpose_scale(x, self.xT, None)
            ext.transpose_scale(dict_w, self.WT, self.inv_norms)
            if self.tied:
                ext.enc_fwd2(self.xT, self.WT, bias, self.c, self.loss_parts, self.fired, 0, bk, prio,
                             dict_sizes=self.dict_sizes)
            else:
                ext.transpose_scale(enc, self.WencT, None)
                ext.enc_fwd2(self.xT, self.WencT, bias, self.c, self.loss_parts, self.fired, 0, bk, prio,
                             dict_sizes=self.dict_sizes)
            ext.dec_fwd(self.c, dict_w, self.inv_norms, x, self.r, self.loss_parts, bk_dec, prio)
            ext.transpose_scale(self.r, self.rT, None)
            ext.gc2(self.rT, self.WT, self.c, self.l1_alpha, self.gpre, self.g_bias, bk, prio)
        else:
            # transpose-in-staging GEMMs (no separate transpose kernels)
            enc_inv = self.inv_norms if self.tied else None
            mode = 3 if self.reverse else 0
            ext.enc_fwd(x, enc, bias, enc_inv, self.c, self.loss_parts, self.fired, mode, bk, prio, bn_enc,
                        dict_sizes=self.dict_sizes)
            ext.dec_fwd(self.c, dict_w, self.inv_norms, x, self.r, self.loss_parts, bk_dec, prio, bn)
            ext.gc(self.r, dict_w, self.inv_norms, self.c, self.l1_alpha, self.gpre, self.g_bias, bk, prio,
                   gc_mode=1 if self.reverse else 0, bn=bn_enc, accumulate=False)

        if on_grads is not None:
            on_grads([self.g_bias])  # final after k_gc

        gscale = 2.0 / (B * d)
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
                ext.grad_w(self.gpre[sl], x, self.gw[sl], 1.0, 1.0, bk_gw, prio, bn)
                on_grads([self.gw[sl]])
        elif self.tied:
            ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio, bn)
            ext.grad_w(self.gpre, x, self.gw, 1.0, 1.0, bk_gw, prio, bn)
            if on_grads is not None:  # M == 1: single unchunked grad tensor
                on_grads([self.gw])
        else:
            ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio, bn)
            if on_grads is not None:
                on_grads([self.gw])
            ext.grad_w(self.gpre, x, self.gw_enc, 1.0, 0.0, bk_gw, prio, bn)
            if on_grads is not None:
                on_grads([self.gw_enc])
        return B

    def update_phase(self, B: int):
        """Adam updates (projection through the renorm for the dictionary)."""
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params

        if self.tied:
            ext.project_adam(p["encoder"], self.gw, self.norms,
                             st["mu"]["encoder"], st["nu"]["encoder"], step_no,
                             self.n_dict, self.lr, self.beta1, self.beta2,
                             self.eps, EPS_NORM, True, lr_mult=self.lr_mult)
        else:
            ext.project_adam(p["decoder"], self.gw, self.norms,
                             st["mu"]["decoder"], st["nu"]["decoder"], step_no,
                             self.n_dict, self.lr, self.beta1, self.beta2,
                             self.eps, EPS_NORM, True, lr_mult=self.lr_mult)
            ext.project_adam(p["encoder"], self.gw_enc, self.norms,
                             st["mu"]["encoder"], st["nu"]["encoder"], step_no,
                             self.n_dict, self.lr, self.beta1, self.beta2,
                             self.eps, EPS_NORM, False, lr_mult=self.lr_mult)
        ext.bias_adam(p["encoder_bias"], self.g_bias, self.bias_decay,
                      st["mu"]["encoder_bias"], st["nu"]["encoder_bias"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps,
                      lr_mult=self.lr_mult)

    def _loss_data(self, B: int):
        d = self.d_act
        mse = self.loss_parts[:, 0] / (B * d)
        l1 = self.l1_alpha * self.loss_parts[:, 1] / B
        if self.masked:  # masked losses carry no bias-decay term
            return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}
        bias = self.ens.params["encoder_bias"]
        l_bd = self.bias_decay * torch.norm(bias, 2, dim=-1)
        total = mse + l1 + l_bd
        return {"loss": total, "l_reconstruction": mse, "l_l1": l1, "l_bias_decay": l_bd}

    # -- public ---------------------------------------------------------------
    def _capture(self, x: torch.Tensor) -> None:
        try:
            self.x_static = x.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                B = self.grads_phase(self.x_static)
                self.update_phase(B)
            self._graph = g
        except Exception as e:  # noqa: BLE001 - graphs are an optimization only
            print(f"[hip_step] hipGraph capture failed ({e}); staying eager")
            self.use_graph = False
            self._graph = None

    def step(self, minibatches: torch.Tensor, expand_dims: bool = True):
        if not expand_dims:
            raise NotImplementedError("per-model batches not supported by the HIP step")
        B = minibatches.shape[0]
        if self.use_graph:
            if self._B == B and self._graph is None and self._eager_steps >= 2:
                self._capture(minibatches.contiguous())
            if self._graph is not None:
                self.x_static.copy_(minibatches)
                self._graph.replay()
                return self._loss_data(B), {"c": self.c}
        B = self.grads_phase(minibatches)
        self.update_phase(B)
        self._eager_steps += 1
        return self._loss_data(B), {"c": self.c}

    def dp_grad_tensors(self):
        """Tensors to all-reduce for data parallelism (average across ranks)."""
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

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)

    def _alloc(self, B: int):
        super()._alloc(B)
        M, n, d = self.n_models, self.n_dict, self.d_act
        dev = self.ens.params["encoder"].device
        self.xc = torch.empty(M, B, d, device=dev)
        self.g_center = torch.empty(M, d, device=dev)
        self.zero_decay = torch.zeros_like(self.bias_decay)
        self.kc["staging"] = "t"

    def grads_phase(self, x: torch.Tensor, on_grads=None):
        ens, ext = self.ens, self.ext
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)
        x = x.contiguous()
        p = ens.params
        enc = p["encoder"]
        bias = p["encoder_bias"]
        center = p["center"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_gw = self.kc["bk_grad_w"] or bk

        self.loss_parts.zero_()
        self.g_bias.zero_()

        torch.sub(x.unsqueeze(0), center.unsqueeze(1), out=self.xc)
        ext.row_norms(enc, self.norms, self.inv_norms, EPS_NORM)
        ext.enc_fwd(self.xc, enc, bias, self.inv_norms, self.c,
                    self.loss_parts, self.fired, 0, bk, prio)
        ext.dec_fwd(self.c, enc, self.inv_norms, self.xc, self.r,
                    self.loss_parts, self.kc["bk_dec"] or bk, prio)
        ext.gc(self.r, enc, self.inv_norms, self.c, self.l1_alpha,
               self.gpre, self.g_bias, bk, prio)

        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.gpre, self.xc, self.gw, 1.0, 1.0, bk_gw, prio)
        # center gradient from existing reductions (docstring derivation);
        # column sum via the coalesced k_colsum kernel
        ext.colsum(self.r, self.g_center, gscale)
        self.g_center.sub_(torch.einsum("mn,mnd->md", self.g_bias * self.inv_norms, enc))
        if on_grads is not None:
            on_grads([self.gw, self.g_bias, self.g_center])
        return B

    def update_phase(self, B: int):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params
        ext.project_adam(p["encoder"], self.gw, self.norms,
                         st["mu"]["encoder"], st["nu"]["encoder"], step_no,
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, EPS_NORM, True, lr_mult=self.lr_mult)
        ext.bias_adam(p["encoder_bias"], self.g_bias, self.zero_decay,
                      st["mu"]["encoder_bias"], st["nu"]["encoder_bias"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps,
                      lr_mult=self.lr_mult)
        ext.bias_adam(p["center"], self.g_center, self.zero_decay,
                      st["mu"]["center"], st["nu"]["center"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps)

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        l1 = self.l1_alpha * self.loss_parts[:, 1] / B
        return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}

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

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)
        b = ensemble.buffers
        rot = b["center_rot"].detach().float()
        scale = b["center_scale"].detach().float()
        self.trans = b["center_trans"].detach().float().contiguous()
        # result[b, c] = sum_u (x-t)[b, u] * rot[c, u] * s[c]
        self.Wc = (rot * scale.unsqueeze(-1)).transpose(1, 2).contiguous()  # [M, d, d]

    def _alloc(self, B: int):
        super()._alloc(B)
        M, n, d = self.n_models, self.n_dict, self.d_act
        dev = self.ens.params["encoder"].device
        self.xsub = torch.empty(M, B, d, device=dev)
        self.xc = torch.empty(M, B, d, device=dev)
        # the per-model-x-stride kernels live in the "t" staging path
        self.kc["staging"] = "t"

    def grads_phase(self, x: torch.Tensor, on_grads=None):
        ens, ext = self.ens, self.ext
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)
        x = x.contiguous()
        p = ens.params
        enc = p["encoder"]
        bias = p["encoder_bias"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_gw = self.kc["bk_grad_w"] or bk

        self.loss_parts.zero_()
        self.g_bias.zero_()

        torch.sub(x.unsqueeze(0), self.trans.unsqueeze(1), out=self.xsub)
        torch.bmm(self.xsub, self.Wc, out=self.xc)  # library GEMM: plain batched matmul

        ext.row_norms(enc, self.norms, self.inv_norms, EPS_NORM)
        ext.enc_fwd(self.xc, enc, bias, self.inv_norms, self.c,
                    self.loss_parts, self.fired, 0, bk, prio)
        ext.dec_fwd(self.c, enc, self.inv_norms, self.xc, self.r,
                    self.loss_parts, self.kc["bk_dec"] or bk, prio)
        ext.gc(self.r, enc, self.inv_norms, self.c, self.l1_alpha,
               self.gpre, self.g_bias, bk, prio)

        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.gpre, self.xc, self.gw, 1.0, 1.0, bk_gw, prio)
        if on_grads is not None:
            on_grads([self.gw, self.g_bias])
        return B
    # update_phase / _loss_data: inherited tied versions (incl. bias decay)


class HipPositiveStep(HipSAEStep):
    """Fused step for FunctionalPositiveTiedSAE (mlp_tests.py:68-125):
    the tied pipeline runs on Wc = clamp(W, 0) and the shifted input
    x' = x + 0.18; the projected gradient is masked by the clamp derivative
    before Adam updates the raw (signed) encoder."""

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)

    def _alloc(self, B: int):
        super()._alloc(B)
        M, n, d = self.n_models, self.n_dict, self.d_act
        dev = self.ens.params["encoder"].device
        self.Wc = torch.empty(M, n, d, device=dev)
        self.x_shift = torch.empty(B, d, device=dev)
        self.kc["staging"] = "t"

    def grads_phase(self, x: torch.Tensor, on_grads=None):
        from sparse_coding_amd.models.positive import INPUT_SHIFT

        ens, ext = self.ens, self.ext
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)
        x = x.contiguous()
        p = ens.params
        enc = p["encoder"]
        bias = p["encoder_bias"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_gw = self.kc["bk_grad_w"] or bk

        self.loss_parts.zero_()
        self.g_bias.zero_()

        torch.clamp(enc, min=0.0, out=self.Wc)
        torch.add(x, INPUT_SHIFT, out=self.x_shift)
        ext.row_norms(self.Wc, self.norms, self.inv_norms, EPS_NORM)
        ext.enc_fwd(self.x_shift, self.Wc, bias, self.inv_norms, self.c,
                    self.loss_parts, self.fired, 0, bk, prio)
        ext.dec_fwd(self.c, self.Wc, self.inv_norms, self.x_shift, self.r,
                    self.loss_parts, self.kc["bk_dec"] or bk, prio)
        ext.gc(self.r, self.Wc, self.inv_norms, self.c, self.l1_alpha,
               self.gpre, self.g_bias, bk, prio)

        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.gpre, self.x_shift, self.gw, 1.0, 1.0, bk_gw, prio)
        if on_grads is not None:
            on_grads([self.gw, self.g_bias])
        return B

    def update_phase(self, B: int):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params
        ext.project_adam(p["encoder"], self.gw, self.norms,
                         st["mu"]["encoder"], st["nu"]["encoder"], step_no,
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, EPS_NORM, True,
                         w_used=self.Wc, clamp_mask=True, lr_mult=self.lr_mult)
        ext.bias_adam(p["encoder_bias"], self.g_bias, self.bias_decay,
                      st["mu"]["encoder_bias"], st["nu"]["encoder_bias"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps,
                      lr_mult=self.lr_mult)


class HipThresholdStep(HipSAEStep):
    """Fused step for FunctionalThresholdingSAE.

    Tied dictionary with a learned soft-threshold gate instead of bias+ReLU
    (reference sae_ensemble.py:232-289): the encoder GEMM runs with a gate
    epilogue (k_enc_fwd_t mode 2) that keeps u = (c+gain)/max(a^2,eps) for
    the backward, and k_gc_thresh_t pushes dL/dcode through g'(u) while
    accumulating the per-feature gain/scale gradients as column sums.
    Weight grads + renorm-projected Adam are the tied-SAE kernels.
    """

    def __init__(self, ensemble, ext):
        super().__init__(ensemble, ext, tied=True)

    def _alloc(self, B: int):
        super()._alloc(B)
        M, n, d = self.n_models, self.n_dict, self.d_act
        dev = self.ens.params["encoder"].device
        self.u = torch.empty(M, B, n, device=dev)
        self.g_gain = torch.zeros(M, n, device=dev)
        self.g_scale = torch.zeros(M, n, device=dev)
        self.dummy_bias = torch.zeros(M, n, device=dev)
        self.zero_decay = torch.zeros_like(self.bias_decay)
        # the gate epilogue lives only in the transpose-in-staging kernels
        self.kc["staging"] = "t"

    def grads_phase(self, x: torch.Tensor, on_grads=None):
        ens, ext = self.ens, self.ext
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)
        x = x.contiguous()
        p = ens.params
        enc = p["encoder"]
        a = p["activation_scale"]
        gain = p["activation_gain"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_gw = self.kc["bk_grad_w"] or bk

        self.loss_parts.zero_()
        self.g_gain.zero_()
        self.g_scale.zero_()

        ext.row_norms(enc, self.norms, self.inv_norms, EPS_NORM)
        ext.enc_fwd(x, enc, self.dummy_bias, self.inv_norms, self.c,
                    self.loss_parts, self.fired, 2, bk, prio,
                    act_scale=a, act_gain=gain, u_out=self.u)
        ext.dec_fwd(self.c, enc, self.inv_norms, x, self.r, self.loss_parts,
                    self.kc["bk_dec"] or bk, prio)
        ext.gc_thresh(self.r, enc, self.inv_norms, self.c, self.u, a,
                      self.l1_alpha, self.gpre, self.g_gain, self.g_scale, bk, prio)

        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.gpre, x, self.gw, 1.0, 1.0, bk_gw, prio)
        if on_grads is not None:
            on_grads([self.gw, self.g_gain, self.g_scale])
        return B

    def update_phase(self, B: int):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params
        zero_decay = self.zero_decay
        ext.project_adam(p["encoder"], self.gw, self.norms,
                         st["mu"]["encoder"], st["nu"]["encoder"], step_no,
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, EPS_NORM, True, lr_mult=self.lr_mult)
        ext.bias_adam(p["activation_scale"], self.g_scale, zero_decay,
                      st["mu"]["activation_scale"], st["nu"]["activation_scale"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps,
                      lr_mult=self.lr_mult)
        ext.bias_adam(p["activation_gain"], self.g_gain, zero_decay,
                      st["mu"]["activation_gain"], st["nu"]["activation_gain"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps,
                      lr_mult=self.lr_mult)

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        l1 = self.l1_alpha * self.loss_parts[:, 1] / B
        return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}

    def dp_grad_tensors(self):
        return [self.gw, self.g_gain, self.g_scale]


class HipLISTAStep:
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
        self.ens = ensemble
        self.ext = ext
        p = ensemble.params
        self.n_models, self.n_dict, self.d_act = p["decoder"].shape
        self.n_layers = len(p["encoder_layers"])

        opt = ensemble.optimizer_kwargs
        self.lr = float(opt.get("lr", 1e-3))
        betas = opt.get("betas", (0.9, 0.999))
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.eps = float(opt.get("eps", 1e-8))
        if getattr(ensemble.optimizer_func, "__name__", "adam") != "adam":
            raise RuntimeError("fused HIP step supports adam only")
        self.l1_alpha = ensemble.buffers["l1_alpha"].detach().reshape(self.n_models).contiguous()
        self._B = None
        import os as _os

        self.use_graph = _os.environ.get("SPARSE_CODING_AMD_NO_GRAPH") != "1"
        self._graph = None
        self._eager_steps = 0

    def _alloc(self, B: int):
        from sparse_coding_amd.ops.kconfig import kernel_config

        self.kc = kernel_config()
        M, n, d, L = self.n_models, self.n_dict, self.d_act, self.n_layers
        dev = self.ens.params["decoder"].device
        f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        self.norms, self.inv_norms = f(M, n), f(M, n)
        self.ones_mn = torch.ones(M, n, device=dev)
        self.zeros_bd = torch.zeros(B, d, device=dev)
        self.scratch_lp = f(M, 2)
        self.loss_parts = f(M, 2)
        self.fired = torch.zeros(M, n, device=dev)
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
        self.carry_a = torch.zeros(M, B, n, device=dev)
        self.carry_b = torch.zeros(M, B, n, device=dev)
        self.sgn = f(M, B, n)
        self.g_e = f(M, B, d)
        self.gA = f(M, n, d)
        self.gW = [f(M, n, d) for _ in range(L)]
        self.g_theta = [f(M, n) for _ in range(L)]
        self.g_rho = [f(M) for _ in range(L)]
        self.scratch_mn = f(M, n)
        self.zero_decay = torch.zeros(M, device=dev)
        self._B = B
        self._graph = None
        self._eager_steps = 0

    def grads_phase(self, x_in: torch.Tensor, on_grads=None):
        ens, ext = self.ens, self.ext
        M, n, d, L = self.n_models, self.n_dict, self.d_act, self.n_layers
        B = x_in.shape[0]
        if self._B != B:
            self._alloc(B)
        b = x_in.contiguous()
        p = ens.params
        A = p["decoder"]
        layers = p["encoder_layers"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_dec = self.kc["bk_dec"] or bk
        bk_gw = self.kc["bk_grad_w"] or bk

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
            if on_grads is not None:
                on_grads([self.gW[l], self.g_theta[l], self.g_rho[l]])
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
        if on_grads is not None:
            on_grads([self.gA])
        return B

    def update_phase(self, B: int):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params
        ext.project_adam(p["decoder"], self.gA, self.norms,
                         st["mu"]["decoder"], st["nu"]["decoder"], step_no,
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, EPS_NORM, True)
        for l in range(self.n_layers):
            ext.project_adam(p["encoder_layers"][l]["W"], self.gW[l], self.norms,
                             st["mu"]["encoder_layers"][l]["W"],
                             st["nu"]["encoder_layers"][l]["W"], step_no,
                             self.n_dict, self.lr, self.beta1, self.beta2,
                             self.eps, EPS_NORM, False)
            ext.bias_adam(p["encoder_layers"][l]["theta"], self.g_theta[l],
                          self.zero_decay,
                          st["mu"]["encoder_layers"][l]["theta"],
                          st["nu"]["encoder_layers"][l]["theta"],
                          step_no, self.lr, self.beta1, self.beta2, self.eps)
            # clamp gate on rho (identical on every DP rank)
            rho = p["encoder_layers"][l]["rho"].reshape(self.n_models)
            self.g_rho[l].mul_(((rho > 0.0) & (rho < 1.0)).float())
            self._apply_rho_adam(l, step_no)

    def _apply_rho_adam(self, l, step_no):
        st = self.ens.optim_states
        rho = self.ens.params["encoder_layers"][l]["rho"]
        mu = st["mu"]["encoder_layers"][l]["rho"]
        nu = st["nu"]["encoder_layers"][l]["rho"]
        g = self.g_rho[l].reshape(rho.shape)
        t = step_no.reshape(rho.shape)
        mu.mul_(self.beta1).add_(g, alpha=1 - self.beta1)
        nu.mul_(self.beta2).addcmul_(g, g, value=1 - self.beta2)
        bc1 = 1 - torch.pow(self.beta1, t)
        bc2 = 1 - torch.pow(self.beta2, t)
        rho.sub_(self.lr * (mu / bc1) / ((nu / bc2).sqrt() + self.eps))

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        self.ext.colsum(self.y[self.n_layers], self.scratch_mn, absval=True)
        l1 = self.l1_alpha * self.scratch_mn.sum(dim=1) / B
        return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}

    def _capture(self, x: torch.Tensor) -> None:
        try:
            self.x_static = x.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                B = self.grads_phase(self.x_static)
                self.update_phase(B)
            self._graph = g
        except Exception as e:  # noqa: BLE001 - graphs are an optimization only
            print(f"[hip_step] hipGraph capture failed ({e}); staying eager")
            self.use_graph = False
            self._graph = None

    def step(self, minibatches: torch.Tensor, expand_dims: bool = True):
        if not expand_dims:
            raise NotImplementedError("per-model batches not supported by the HIP step")
        B = minibatches.shape[0]
        if self.use_graph:
            if self._B == B and self._graph is None and self._eager_steps >= 2:
                self._capture(minibatches.contiguous())
            if self._graph is not None:
                self.x_static.copy_(minibatches)
                self._graph.replay()
                return self._loss_data(B), {"c": self.y[self.n_layers]}
        B = self.grads_phase(minibatches)
        self.update_phase(B)
        self._eager_steps += 1
        return self._loss_data(B), {"c": self.y[self.n_layers]}

    def dp_grad_tensors(self):
        return [self.gA] + self.gW + self.g_theta + self.g_rho


class HipResidualDenoisingStep:
    """Fused step for FunctionalResidualDenoisingSAE
    (residual_denoising_autoencoder.py:125-201): x0 = b A_hat^T, then
    L residual blocks x' = relu(x + theta_l) W_l^T + x (W_l is [n, n]),
    c = relu(x_L + bias).  Same kernel-orchestration recipe as HipLISTAStep;
    all GEMMs (including the [n,n] layer products) run on the MFMA kernels.
    """

    def __init__(self, ensemble, ext):
        self.ens = ensemble
        self.ext = ext
        p = ensemble.params
        self.n_models, self.n_dict, self.d_act = p["decoder"].shape
        self.n_layers = len(p["encoder_layers"])
        opt = ensemble.optimizer_kwargs
        self.lr = float(opt.get("lr", 1e-3))
        betas = opt.get("betas", (0.9, 0.999))
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.eps = float(opt.get("eps", 1e-8))
        if getattr(ensemble.optimizer_func, "__name__", "adam") != "adam":
            raise RuntimeError("fused HIP step supports adam only")
        self.l1_alpha = ensemble.buffers["l1_alpha"].detach().reshape(self.n_models).contiguous()
        self._B = None

    def _alloc(self, B: int):
        from sparse_coding_amd.ops.kconfig import kernel_config

        self.kc = kernel_config()
        M, n, d, L = self.n_models, self.n_dict, self.d_act, self.n_layers
        dev = self.ens.params["decoder"].device
        f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        self.norms, self.inv_norms = f(M, n), f(M, n)
        self.ones_mn = torch.ones(M, n, device=dev)
        self.zeros_bn = torch.zeros(B, n, device=dev)
        self.scratch_lp = f(M, 2)
        self.loss_parts = f(M, 2)
        self.fired = torch.zeros(M, n, device=dev)
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
        self.zero_decay = torch.zeros(M, device=dev)
        self._B = B

    def grads_phase(self, x_in: torch.Tensor, on_grads=None):
        ens, ext = self.ens, self.ext
        M, n, d, L = self.n_models, self.n_dict, self.d_act, self.n_layers
        B = x_in.shape[0]
        if self._B != B:
            self._alloc(B)
        b = x_in.contiguous()
        p = ens.params
        A = p["decoder"]
        layers = p["encoder_layers"]
        bias = p["encoder_bias"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_dec = self.kc["bk_dec"] or bk
        bk_gw = self.kc["bk_grad_w"] or bk

        self.loss_parts.zero_()
        self.g_bias.zero_()
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
        torch.add(self.xs[L], bias.unsqueeze(1), out=self.c)
        self.c.clamp_(min=0.0)

        ext.dec_fwd(self.c, A, self.inv_norms, b, self.rr, self.loss_parts, bk_dec, prio)
        # c >= 0, so the L1 sum is a column sum + tiny [M, n] reduce; the
        # torch sum(dim=(1,2)) dispatched a 1.79 ms strided reduce
        # (profiles/r02_residual_kernel_stats.csv)
        ext.colsum(self.c, self.scratch_mn)
        self._l1_sum = self.scratch_mn.sum(dim=1)

        # backward: g_c via k_gc (relu mask + l1 term + bias colsum, K=d)
        ext.gc(self.rr, A, self.inv_norms, self.c, self.l1_alpha,
               self.g_x, self.g_bias, bk, prio)
        gscale = 2.0 / (B * d)
        ext.grad_w(self.c, self.rr, self.gA, gscale, 0.0, bk_gw, prio)

        for l in range(L - 1, -1, -1):
            W_l, theta = layers[l]["W"], layers[l]["theta"]
            # g_W_l = g_x'^T h
            ext.grad_w(self.g_x, self.hs[l], self.gW[l], 1.0, 0.0, bk_gw, prio)
            if on_grads is not None:
                on_grads([self.gW[l]])
            # g_h = g_x' @ W_l  ([M,B,n] x [M,n,n])
            ext.dec_fwd(self.g_x, W_l, self.ones_mn, self.zeros_bn, self.g_h,
                        self.scratch_lp, bk_dec, prio)
            # relu(x + theta) backward
            self.g_h.mul_((self.hs[l] > 0).float())
            # column sum via k_colsum: torch.sum(dim=1) dispatches a strided
            # reduce at ~140 GB/s (rocprof r02_residual_kernel_stats: 1.79 ms
            # = 5% of the step); the coalesced-row kernel streams the same
            # bytes at HBM rate
            ext.colsum(self.g_h, self.g_theta[l])
            if on_grads is not None:
                on_grads([self.g_theta[l]])
            self.g_x.add_(self.g_h)  # residual skip + through-layer paths

        # x0 = b A_hat^T
        ext.grad_w(self.g_x, b, self.gA, 1.0, 1.0, bk_gw, prio)
        if on_grads is not None:
            on_grads([self.gA, self.g_bias])
        return B

    def update_phase(self, B: int):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params
        ext.project_adam(p["decoder"], self.gA, self.norms,
                         st["mu"]["decoder"], st["nu"]["decoder"], step_no,
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, EPS_NORM, True)
        for l in range(self.n_layers):
            ext.project_adam(p["encoder_layers"][l]["W"], self.gW[l], self.norms,
                             st["mu"]["encoder_layers"][l]["W"],
                             st["nu"]["encoder_layers"][l]["W"], step_no,
                             self.n_dict, self.lr, self.beta1, self.beta2,
                             self.eps, EPS_NORM, False)
            ext.bias_adam(p["encoder_layers"][l]["theta"], self.g_theta[l],
                          self.zero_decay,
                          st["mu"]["encoder_layers"][l]["theta"],
                          st["nu"]["encoder_layers"][l]["theta"],
                          step_no, self.lr, self.beta1, self.beta2, self.eps)
        ext.bias_adam(p["encoder_bias"], self.g_bias, self.zero_decay,
                      st["mu"]["encoder_bias"], st["nu"]["encoder_bias"],
                      step_no, self.lr, self.beta1, self.beta2, self.eps)

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        l1 = self.l1_alpha * self._l1_sum / B
        return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}

    def step(self, minibatches: torch.Tensor, expand_dims: bool = True):
        if not expand_dims:
            raise NotImplementedError
        B = self.grads_phase(minibatches)
        self.update_phase(B)
        return self._loss_data(B), {"c": self.c}

    def dp_grad_tensors(self):
        return [self.gA, self.g_bias] + self.gW + self.g_theta


class HipSemilinearStep:
    """Fused step for SemiLinearSAE (semilinear_autoencoder.py:14-83): a
    2-layer relu MLP encoder + normalized linear decoder.  The top-layer
    backward IS k_gc (relu mask + l1 + bias column sums); the hidden layer
    is one more GEMM pair.
    """

    def __init__(self, ensemble, ext):
        self.ens = ensemble
        self.ext = ext
        p = ensemble.params
        self.n_models, self.n_dict, self.d_act = p["decoder"].shape
        self.hidden = p["encoder_layers"][0]["weight"].shape[1]  # [M, h, d] -> h
        assert len(p["encoder_layers"]) == 2
        opt = ensemble.optimizer_kwargs
        self.lr = float(opt.get("lr", 1e-3))
        betas = opt.get("betas", (0.9, 0.999))
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.eps = float(opt.get("eps", 1e-8))
        if getattr(ensemble.optimizer_func, "__name__", "adam") != "adam":
            raise RuntimeError("fused HIP step supports adam only")
        self.l1_alpha = ensemble.buffers["l1_alpha"].detach().reshape(self.n_models).contiguous()
        self._B = None

    def _alloc(self, B: int):
        from sparse_coding_amd.ops.kconfig import kernel_config

        self.kc = kernel_config()
        M, n, d, h = self.n_models, self.n_dict, self.d_act, self.hidden
        dev = self.ens.params["decoder"].device
        f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        self.norms, self.inv_norms = f(M, n), f(M, n)
        self.ones_mh = torch.ones(M, h, device=dev)
        self.zeros_bh = torch.zeros(B, h, device=dev)
        self.scratch_lp = f(M, 2)
        self.loss_parts = f(M, 2)
        self.fired = torch.zeros(M, n, device=dev)
        self.fired_h = torch.zeros(M, h, device=dev)
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
        self.zero_decay = torch.zeros(M, device=dev)
        self._B = B

    def grads_phase(self, x_in: torch.Tensor, on_grads=None):
        ens, ext = self.ens, self.ext
        B = x_in.shape[0]
        if self._B != B:
            self._alloc(B)
        b = x_in.contiguous()
        p = ens.params
        A = p["decoder"]
        l1p, l2p = p["encoder_layers"]
        bk, prio = self.kc["bk"], self.kc["prio"]
        bk_dec = self.kc["bk_dec"] or bk
        bk_gw = self.kc["bk_grad_w"] or bk

        self.loss_parts.zero_()
        self.g_b2.zero_()
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
               self.g_c, self.g_b2, bk, prio)
        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.rr, self.gA, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.g_c, self.h1, self.gW2, 1.0, 0.0, bk_gw, prio)
        # g_h1 = (g_c W2) * [h1 > 0]
        ext.dec_fwd(self.g_c, l2p["weight"], self.ones_mh, self.zeros_bh,
                    self.g_h, self.scratch_lp, bk_dec, prio)
        self.g_h.mul_((self.h1 > 0).float())
        # strided-reduce -> k_colsum (9% of the semilinear step,
        # rocprof r02_semilinear_kernel_stats)
        ext.colsum(self.g_h, self.g_b1)
        ext.grad_w(self.g_h, b, self.gW1, 1.0, 0.0, bk_gw, prio)
        if on_grads is not None:
            on_grads([self.gA, self.gW2, self.gW1, self.g_b2, self.g_b1])
        return B

    def update_phase(self, B: int):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        step_no = st["step"]
        p = ens.params
        ext.project_adam(p["decoder"], self.gA, self.norms,
                         st["mu"]["decoder"], st["nu"]["decoder"], step_no,
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, EPS_NORM, True)
        for li, (gW, gb) in enumerate(((self.gW1, self.g_b1), (self.gW2, self.g_b2))):
            lay = p["encoder_layers"][li]
            ext.project_adam(lay["weight"], gW, self.norms,
                             st["mu"]["encoder_layers"][li]["weight"],
                             st["nu"]["encoder_layers"][li]["weight"], step_no,
                             gW.shape[1], self.lr, self.beta1, self.beta2,
                             self.eps, EPS_NORM, False)
            ext.bias_adam(lay["bias"], gb, self.zero_decay,
                          st["mu"]["encoder_layers"][li]["bias"],
                          st["nu"]["encoder_layers"][li]["bias"],
                          step_no, self.lr, self.beta1, self.beta2, self.eps)

    def _loss_data(self, B: int):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        l1 = self.l1_alpha * self._l1_sum / B
        return {"loss": mse + l1, "l_reconstruction": mse, "l_l1": l1}

    def step(self, minibatches: torch.Tensor, expand_dims: bool = True):
        if not expand_dims:
            raise NotImplementedError
        B = self.grads_phase(minibatches)
        self.update_phase(B)
        return self._loss_data(B), {"c": self.c}

    def dp_grad_tensors(self):
        return [self.gA, self.gW1, self.gW2, self.g_b1, self.g_b2]


class HipTopKStep:
    """Fused TopK-encoder training step.

    Same GEMM pipeline as the tied SAE but: raw-score encoder (no bias/relu),
    per-row top-k selection + scatter + relu between encode and decode, no L1
    term, and the dictionary normalization has NO eps clamp
    (reference topk_encoder.py:31).  The per-model k lives in
    buffers["sparsity"]; selection runs as one torch.topk per model.
    """

    EPS = 1e-30  # un-clamped normalization (reference divides by the raw norm)

    def __init__(self, ensemble, ext):
        self.ens = ensemble
        self.ext = ext
        p = ensemble.params
        self.n_models, self.n_dict, self.d_act = p["dict"].shape
        dev = p["dict"].device
        self.ks = [int(k) for k in ensemble.buffers["sparsity"].reshape(-1).tolist()]
        self.ks_i32 = torch.tensor(self.ks, device=dev, dtype=torch.int32)
        self.zero_l1 = torch.zeros(self.n_models, device=dev)
        self.dummy_bias = torch.zeros(self.n_models, self.n_dict, device=dev)
        self.lr_mult = torch.ones(self.n_models, self.n_dict, device=dev)

        opt = ensemble.optimizer_kwargs
        self.lr = float(opt.get("lr", 1e-3))
        betas = opt.get("betas", (0.9, 0.999))
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.eps = float(opt.get("eps", 1e-8))
        name = getattr(ensemble.optimizer_func, "__name__", "adam")
        if name != "adam":
            raise RuntimeError(f"fused HIP step supports adam only, got {name}")
        self._B = None
        import os as _os

        self.use_graph = _os.environ.get("SPARSE_CODING_AMD_NO_GRAPH") != "1"
        self._graph = None
        self._eager_steps = 0

    def _alloc(self, B):
        from sparse_coding_amd.ops.kconfig import kernel_config

        self.kc = kernel_config()
        M, n, d = self.n_models, self.n_dict, self.d_act
        dev = self.ens.params["dict"].device
        f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        self.scores = f(M, B, n)
        self.c = f(M, B, n)
        self.gpre = f(M, B, n)
        self.r = f(M, B, d)
        self.norms = f(M, n)
        self.inv_norms = f(M, n)
        self.loss_parts = f(M, 2)
        self.fired = torch.zeros(M, n, device=dev)
        self.g_bias_scratch = f(M, n)
        self.gw = f(M, n, d)
        self._B = B
        self._graph = None
        self._eager_steps = 0

    def grads_phase(self, x):
        ens, ext = self.ens, self.ext
        B = x.shape[0]
        if self._B != B:
            self._alloc(B)
        x = x.contiguous()
        W = ens.params["dict"]

        self.loss_parts.zero_()
        self.g_bias_scratch.zero_()

        kc = self.kc
        bk, prio = kc["bk"], kc["prio"]
        bk_dec = kc["bk_dec"] or bk
        bk_gw = kc["bk_grad_w"] or bk
        ext.row_norms(W, self.norms, self.inv_norms, self.EPS)
        ext.enc_fwd(x, W, self.dummy_bias, self.inv_norms,
                    self.scores, self.loss_parts, self.fired, 1, bk, prio)
        # exact per-row radix top-k + scatter + fired counts in ONE kernel
        # (k_topk_select) — replaces the torch.topk/scatter chain
        ext.topk_select(self.scores, self.c, self.fired, self.ks_i32)

        ext.dec_fwd(self.c, W, self.inv_norms, x, self.r, self.loss_parts, bk_dec, prio)
        ext.gc(self.r, W, self.inv_norms, self.c, self.zero_l1,
               self.gpre, self.g_bias_scratch, bk, prio)
        gscale = 2.0 / (B * self.d_act)
        ext.grad_w(self.c, self.r, self.gw, gscale, 0.0, bk_gw, prio)
        ext.grad_w(self.gpre, x, self.gw, 1.0, 1.0, bk_gw, prio)
        return B

    def update_phase(self, B):
        ens, ext = self.ens, self.ext
        st = ens.optim_states
        st["step"] += 1.0
        ext.project_adam(ens.params["dict"], self.gw, self.norms,
                         st["mu"]["dict"], st["nu"]["dict"], st["step"],
                         self.n_dict, self.lr, self.beta1, self.beta2,
                         self.eps, self.EPS, True, lr_mult=self.lr_mult)

    def _loss_data(self, B):
        mse = self.loss_parts[:, 0] / (B * self.d_act)
        return {"loss": mse}

    def _capture(self, x):
        try:
            self.x_static = x.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                B = self.grads_phase(self.x_static)
                self.update_phase(B)
            self._graph = g
        except Exception as e:  # noqa: BLE001 - graphs are an optimization only
            print(f"[hip_step] hipGraph capture failed ({e}); staying eager")
            self.use_graph = False
            self._graph = None

    def step(self, minibatches, expand_dims=True):
        if not expand_dims:
            # per-model batches not needed: TopK stacks fine on this path
            raise NotImplementedError
        B = minibatches.shape[0]
        if self.use_graph:
            if self._B == B and self._graph is None and self._eager_steps >= 2:
                self._capture(minibatches.contiguous())
            if self._graph is not None:
                self.x_static.copy_(minibatches)
                self._graph.replay()
                return self._loss_data(B), {"c": self.c}
        B = self.grads_phase(minibatches)
        self.update_phase(B)
        self._eager_steps += 1
        return self._loss_data(B), {"c": self.c}

    def dp_grad_tensors(self):
        return [self.gw]
