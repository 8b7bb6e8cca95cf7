"""One training step of Openset R-CNN on the HIP path: forward with saved activations, the six losses, backward through every
trainable layer, SGD with momentum -- the loop body of the reference's trainer (train.py:132-148: `loss_dict = model(data);
losses.backward(); optimizer.step()`) for META_ARCHITECTURE GeneralizedRCNN with [d2] defaults: FrozenBN everywhere, SGD
momentum 0.9, weight decay 1e-4 on weights and biases. MODEL.BACKBONE.FREEZE_AT decides which backbone stages train (`freeze_at`:
0 = stem and res2..res5, 1 = res2..res5, 2 = res3..res5 -- [d2]'s default and the trainer's --, ..., 5 = none; the FPN laterals of
frozen stages still train). A trainable stem keeps its output for the backward (osr_conv2d_fwd stem view + osr_maxpool3x3s2 instead
of the fused osr_stem_maxpool_fwd_raw) and differentiates it with osr_stem_pool_bwd / osr_stem_wgrad (csrc/osr_stem_bwd.hip).

What runs where: every convolution / FC forward, data gradient and weight gradient is an MFMA kernel launch (osr_conv2d_fwd /
osr_conv2d_wgrad), targets, sampling, losses and their gradients, RoIAlign forward/backward, the CF-RPN tail and the update are
the kernels of osr_train_fwd.hip / osr_train_bwd.hip / osr_roi_align.hip. torch is used for memory, views, zero-fills and a few
layout copies of small fp32 matrices (transposes / column padding for the exact-fp32 GEMM of the 5-, 21- and 256-wide heads).

Mixed precision: fp16 (or bf16) activations and activation gradients, fp32 accumulation, fp32 master weights and momentum,
static loss scaling (gradient tensors are multiplied by `loss_scale`, the update divides it out).
Data parallel: one process per GPU; `all_reduce_grads()` sums the single flat fp32 gradient buffer over RCCL (train.py:201-205
wraps the model in DDP) and the update divides by the world size."""
from __future__ import annotations

import collections
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import ops, parallel
from .engine import PYRAMID, RPN_CONV, STEM, OpensetRCNNEngine, loss_types_of, refuse_deform_training
from .weights import R50_BLOCKS, pack_conv_weight, pack_fc1_weight, pack_stem_weight


def warmup_multistep_lr(iteration: int, base_lr: float, steps: Tuple[int, ...], gamma: float = 0.1, warmup_iters: int = 1000,
                        warmup_factor: float = 1.0 / 1000) -> float:
    """[d2] WarmupMultiStepLR (SOLVER.LR_SCHEDULER_NAME default; VOC-COCO yaml: BASE_LR 0.005, STEPS (84000, 116000),
    WARMUP_ITERS 400): linear warm-up of the factor from warmup_factor to 1, then x gamma at every milestone passed."""
    lr = base_lr * gamma ** sum(1 for s in steps if iteration >= s)
    if iteration < warmup_iters:
        alpha = iteration / warmup_iters
        lr *= warmup_factor * (1 - alpha) + alpha
    return lr


class SolverOptions(NamedTuple):
    """What the trainer's update needs beyond group 0's lr / momentum / weight decay (OpensetRCNNTrainer.solver_options; solver.HipSGD
    derives it from its parameter groups). The defaults are one plain SGD group."""
    bias_lr_factor: float = 1.0          # bias group lr / base group lr
    weight_decay_bias: Optional[float] = None  # None: the bias parameters are in the base group
    nesterov: bool = False
    clip: Optional[str] = None           # None, "value" or "norm" ([d2] maybe_add_gradient_clipping, per parameter)
    clip_value: float = 1.0
    norm_type: float = 2.0


class DynamicLossScale:
    """Host half of the overflow guard: one (event, pinned slot) per update, drained IN ORDER. The device half is a flag that
    osr_check_finite clears and the update launch of the iteration reads (a poisoned update changes nothing, no host
    sync). `record(flag)` queues that flag's copy into a slot of its own right after an update; `poll(wait)` applies the verdicts
    of the updates that have finished -- an overflow halves the scale (floor 1.0), `growth_interval` consecutive clean updates
    double it again, never past the configured scale (what torch's GradScaler does) -- so no verdict is ever overwritten however
    far the host runs ahead of the GPU, and the scale is not a one-way ratchet.

    The same slot carries the iteration's PROPOSAL STATUS word (osr_rpn_select's status_flags: non-zero when a predicted box or
    score was Inf / NaN). The reference raises FloatingPointError for that in training (find_top_proposals.py:96-101); here the
    word rides with the overflow verdict -- no extra host sync -- and `poll` raises the same exception when it drains the slot."""

    DIVERGED = "Predicted boxes or scores contain Inf/NaN. Training has diverged."  # find_top_proposals.py:99-101

    def __init__(self, scale: float, growth_interval: int = 2000, device: Optional[torch.device] = None):
        self.scale, self.scale_max, self.growth_interval = float(scale), float(scale), int(growth_interval)
        self.cuda = device is not None and torch.device(device).type == "cuda"
        self.queue: collections.deque = collections.deque()
        self.free: List[torch.Tensor] = []
        self.overflow_steps = 0
        self.clean_steps = 0  # consecutive clean updates since the last overflow / growth

    def record(self, ok_flag: torch.Tensor, proposal_status: Optional[torch.Tensor] = None) -> None:
        """ok_flag: (1,) int32 on the trainer's device, 1 = the update just enqueued was applied, 0 = skipped.
        proposal_status: (1,) int32, osr_rpn_select's status word of the same iteration (0 = every prediction finite)."""
        if self.free:
            slot = self.free.pop()
        else:
            slot = torch.ones((2,), dtype=torch.int32)
            if self.cuda:
                slot = slot.pin_memory()
        slot[0:1].copy_(ok_flag, non_blocking=True)
        if proposal_status is not None:
            slot[1:2].copy_(proposal_status, non_blocking=True)
        else:
            slot[1] = 0
        ev = None
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record()
        self.queue.append((ev, slot, self.scale))  # the scale this update was issued with

    def poll(self, wait: bool = False, lag: int = 0) -> bool:
        """True when at least one of the drained updates had been skipped. lag: leave the newest `lag` updates in the queue
        whatever their state -- with wait=True the call then applies EXACTLY the verdicts of all updates but the newest `lag`,
        a deterministic set (the same on every rank of a data-parallel job), while the host keeps `lag` iterations of run-ahead."""
        any_overflow = False
        while len(self.queue) > lag:
            ev, slot, issued_scale = self.queue[0]
            if ev is not None:
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    break
            self.queue.popleft()
            ok, diverged = int(slot[0]) == 1, int(slot[1]) != 0
            self.free.append(slot)
            if diverged:
                raise FloatingPointError(self.DIVERGED)
            if ok:
                self.clean_steps += 1
                if self.growth_interval > 0 and self.clean_steps >= self.growth_interval and self.scale < self.scale_max:
                    self.scale = min(self.scale_max, self.scale * 2.0)
                    self.clean_steps = 0
            else:
                any_overflow = True
                self.overflow_steps += 1
                self.clean_steps = 0
                # One back-off per overflow EPISODE (GradScaler's behaviour): with a verdict lag the updates issued between the overflow
                # and its verdict ran at the same, too-large scale and overflow as well; they count as skipped steps but do not halve the
                # scale again (it is already below the scale they were issued with).
                if issued_scale <= self.scale:
                    self.scale = max(1.0, self.scale * 0.5)
        return any_overflow


class OpensetRCNNTrainer:
    def __init__(self, params: Dict[str, torch.Tensor], cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device: str = "cuda",
                 lr: float = 0.005, momentum: float = 0.9, weight_decay: float = 1e-4, loss_scale: float = 1024.0, freeze_at: int = 2,
                 frozen_bn: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None, class_map: Optional[torch.Tensor] = None,
                 bucket_bytes: int = 25 << 20, scale_growth_interval: int = 2000, box_head: str = "storage", conv: str = "storage"):
        """params: BN-folded parameters under detectron2 names (what the engine reads). frozen_bn (optional): for convs followed by
        FrozenBatchNorm, name -> (un-folded weight (cout,cin,kh,kw), per-channel scale gamma/sqrt(var+eps)): the trainable parameter
        is the un-folded weight (weight decay acts on it, the chain rule multiplies the kernel's gradient by the scale).
        box_head: how FC1 / FC2 of the box head multiply, forward and backward. "storage" (default): on operands of the storage
        dtype. "split": the reference's fp32 operands from the RoIAlign output on (OpensetRCNNEngine box_head="split") -- pooled, h1 and
        box_feats are saved in fp32, the two layers' forward, data gradients and weight gradients run on the split-precision kernels
        (ops.linear_split, linear_split_dgrad, linear_split_wgrad: three bf16 MFMA products per term, fp32 sums), fc1.w / fc2.w have
        no low-precision copy: their fp32 masters are re-split into the kernels' bf16 planes after every update.
        conv: "storage" only. The split-precision convolutions (OpensetRCNNEngine conv="split") have no backward: ValueError."""
        freeze_at = self._check_freeze_at(freeze_at)
        refuse_deform_training(cfg or {})  # (a deformable stage has no backward: NotImplementedError naming its key)
        if conv != "storage":
            raise ValueError(f"conv_precision {conv!r}: the split-precision convolutions are an inference mode, training keeps conv=\"storage\"")
        if box_head not in OpensetRCNNEngine.BOX_HEADS:
            raise ValueError(f"box_head must be one of {OpensetRCNNEngine.BOX_HEADS}, got {box_head!r}")
        if box_head != "storage" and not self.SPLIT_BOX_HEAD:
            raise ValueError(f"box_head_precision {box_head!r}: the stock Faster R-CNN engine keeps its box head")
        self.box_head = box_head
        # (tests / diagnostics) set to a dict: _box_head_bwd leaves the gradient it was given (d_bf, a copy), the one it hands to
        # RoIAlign's backward (d_pooled) and what that returns (d_feat, copies of the per-level feature gradients) in it
        self.box_head_probe: Optional[dict] = None
        self.frozen_bn = frozen_bn or {}
        self.row_scale: Dict[str, torch.Tensor] = {}
        self.eng = self._make_engine(params, cfg, dtype, device, class_map) if box_head == "storage" else \
            self._make_engine(params, cfg, dtype, device, class_map, box_head=box_head)
        # the CF-RPN head's backward runs on the sampled anchors only and recomputes their hidden state (osr_rpn_sparse.hip); False:
        # the dense launches of rounds 1-3 (the fused head kernel then also writes the hidden state of every anchor: 0.7 GB)
        self.sparse_rpn_bwd = True
        # None: the list's own capacity (n x 2 x RPN.BATCH_SIZE_PER_IMAGE). A smaller number makes an iteration whose list is longer
        # count as not fitting (tests: the skipped-update path without a pathological sampler)
        self.sparse_rows_cap: Optional[int] = None
        self.dtype, self.device = dtype, self.eng.device
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.scaler = DynamicLossScale(loss_scale, scale_growth_interval, self.eng.device)
        self.freeze_at = freeze_at
        e, dev = self.eng, self.eng.device
        f32 = lambda t: t.detach().float().contiguous().to(dev)  # noqa: E731
        # ---- trainable parameters: fp32 masters (conv / FC weights in the kernels' packed layout) ----
        self.master: Dict[str, torch.Tensor] = {}
        self.lowp: Dict[str, Optional[torch.Tensor]] = {}  # working copy the forward kernels read (None: the master itself is read)
        self.conv_names: List[str] = []
        if freeze_at == 0:
            self._add_stem(params)
        for si, nb in enumerate(R50_BLOCKS):
            if si + 2 <= freeze_at:
                continue
            for b in range(nb):
                pre = f"backbone.bottom_up.res{si + 2}.{b}"
                for cname in (["shortcut"] if b == 0 else []) + ["conv1", "conv2", "conv3"]:
                    self._add_conv(f"{pre}.{cname}", params, bias=False)  # FrozenBN: the folded shift is not a parameter
        # (the masters are laid out in REVERSE order of gradient completion -- backbone bottom-up, FPN coarse to fine, RPN head, box
        # head, the small fp32 heads last -- so that the finished part of the flat gradient buffer grows from its end and the
        # all-reduce buckets of parallel.GradBuckets are contiguous)
        for lvl in (5, 4, 3, 2):
            self._add_conv(f"backbone.fpn_lateral{lvl}", params, bias=True)
            self._add_conv(f"backbone.fpn_output{lvl}", params, bias=True)
        self._add_conv(RPN_CONV, params, bias=True)
        self._add_head_masters(params)
        # ---- one flat gradient buffer (the all-reduce operand), momentum buffers ----
        al = lambda x: (x + 3) // 4 * 4  # noqa: E731  every view starts 16-byte aligned (the kernels use 16-byte accesses)
        total = sum(al(t.numel()) for t in self.master.values())
        self.grad_flat = torch.zeros((total,), dtype=torch.float32, device=dev)
        self.grad: Dict[str, torch.Tensor] = {}
        off, layout = 0, []
        for k, t in self.master.items():
            self.grad[k] = self.grad_flat[off:off + t.numel()].view(t.shape)
            layout.append((k, off, al(t.numel())))
            off += al(t.numel())
        self.buckets = parallel.GradBuckets(self.grad_flat, layout, bucket_bytes)
        self.mom = {k: torch.zeros_like(t) for k, t in self.master.items()}
        # (the stem master is the padded (64, 8, 1, 32) view: its 6 976 padding zeros are not parameters)
        self.num_params = sum(t.numel() for t in self.master.values()) - (16384 - 9408 if STEM + ".w" in self.master else 0)
        # overflow guard: device flag read by the update launch; its host half is self.scaler (DynamicLossScale)
        self._ok = torch.ones((1,), dtype=torch.int32, device=dev)
        self._cside: Optional[torch.cuda.Stream] = None  # stream the gradient buckets' collectives are issued from (see _done)
        self._overlap = False
        self.grads_ready = False
        self._side: Optional[torch.cuda.Stream] = None  # stream of the ground-truth-only part of the forward (anchor targets)
        self.overlap_targets = True
        self._wside: Optional[torch.cuda.Stream] = None  # stream of the weight / bias gradient launches (see _wg)
        self.side_wgrad = True
        self.chain_forward = True  # res3 blocks: conv2 -> conv3 in one launch that also stores conv2's output (osr_conv2d_chain_fwd_ex)
        self._sgd_plans = (None, {})  # (addresses of the buffers, {(bias lr factor, bias weight decay, weight decay, nesterov): plan}), see _sgd_plan
        # [d2] solver options beyond one plain SGD group (SolverOptions: clipping, bias group, Nesterov), set by HipSGD.step;
        # None: the neutral SolverOptions()
        self.solver_options: Optional[SolverOptions] = None
        self._pack_plan = None
        self._pre: Optional[torch.cuda.Stream] = None  # stream of the next batch's frozen prefix (_prefetch_frozen)
        self.backward_concurrency_hint = 2  # launch streams of the backward (data gradients + weight gradients): see step(); 24.0 -> 23.7 ms
        self._prefetched = None                        # (images, (hp, wp), (x, feats), event, images._version)
        # blocks whose weight gradients ride on the main stream (measured with res3.0 / res3.0-1 / all of res3: 25.4-25.5 against 25.5-25.7 ms,
        # inside the run-to-run spread: the backward is bound by the sum of its kernels, not by which stream ends last) -- left empty
        self.wgrad_on_main: set = set()
        self._refresh_derived()

    @property
    def loss_scale(self) -> float:
        return self.scaler.scale

    @loss_scale.setter
    def loss_scale(self, v: float) -> None:  # (load_optimizer_state restores the scale a checkpoint was written with)
        self.scaler.scale = float(v)

    @property
    def overflow_steps(self) -> int:
        return self.scaler.overflow_steps

    @staticmethod
    def _check_freeze_at(freeze_at: int) -> int:
        """[d2] ResNet.freeze semantics: values above 5 act as 5 (the whole bottom-up network frozen), negative values are refused."""
        v = int(freeze_at)
        if v < 0:
            raise ValueError(f"freeze_at must be >= 0, got {v}")
        return min(v, 5)

    SPLIT_BOX_HEAD = True  # whether this trainer has the box_head="split" mode (the stock heads' trainer does not)

    @staticmethod
    def _make_engine(params, cfg, dtype, device, class_map, box_head: str = "storage"):
        return OpensetRCNNEngine(params, cfg, dtype, device, class_map, box_head=box_head)

    def _add_head_masters(self, params) -> None:
        """The masters behind the RPN head's 3x3 conv: CF-RPN tail, box head, predictor, PLN, classifier (in this order: see __init__)."""
        e, dev = self.eng, self.eng.device
        f32 = lambda t: t.detach().float().contiguous().to(dev)  # noqa: E731
        self.master["rpn_tail.w"], self.master["rpn_tail.b"] = e.rpn_wtail, e.rpn_btail  # (5,256): 4 ltrb rows + centerness
        e.rpn_wd, e.rpn_wc, e.rpn_bd, e.rpn_bc = e.rpn_wtail[:4], e.rpn_wtail[4:5], e.rpn_btail[:4], e.rpn_btail[4:5]  # views: one storage
        self.master["fc1.w"] = pack_fc1_weight(params["roi_heads.box_head.fc1.weight"], 256, e.cfg["pooler_resolution"], torch.float32).to(dev)
        self.master["fc1.b"] = e.fc1_b
        self.master["fc2.w"] = f32(params["roi_heads.box_head.fc2.weight"])
        self.master["fc2.b"] = e.fc2_b
        if self.box_head != "split":  # (split: no low-precision copy -- the kernels read the masters' bf16 planes, see _resplit_box_head)
            self.lowp["fc1.w"], self.lowp["fc2.w"] = e.fc1_w, e.fc2_w
        else:
            e.fc1_w = e.fc2_w = None  # (nothing refreshes the engine's storage-dtype copies in this mode, and nothing reads them)
        self.master["pred.w"], self.master["pred.b"] = e.pred_w, e.pred_b
        self.master["enc.w"], self.master["enc.b"] = e.enc_w, e.enc_b
        self.master["dec.w"], self.master["dec.b"] = e.dec_w, e.dec_b
        self.master["cls.w"], self.master["cls.b"] = e.cls_w, e.cls_b
        self.master["protos"] = f32(params["roi_heads.dml.representatives"])

    def _add_stem(self, params) -> None:
        """FREEZE_AT 0: the stem's master in the layout of the stem view the forward kernels read, (64, 8, 1, 32) fp32 (weights.pack_stem_weight:
        the 8th row, the 8th tap and the 4th channel zero). Their gradient is exactly zero (osr_stem_wgrad) and so is their weight decay,
        so the update leaves them zero in the master, the momentum and the working view it refreshes. No backward-data weights: nothing is
        below the stem."""
        e, name = self.eng, STEM
        if name in self.frozen_bn:
            w_unfolded, scale = self.frozen_bn[name]
            self.master[name + ".w"] = pack_stem_weight(w_unfolded, torch.float32).to(e.device)
            self.row_scale[name + ".w"] = scale.detach().float().contiguous().to(e.device)
        else:
            self.master[name + ".w"] = pack_stem_weight(params[name + ".weight"], torch.float32).to(e.device)
        lw = e.w[name + ".w"]
        assert tuple(lw.shape) == (64, 8, 1, 32), "the engine's stem view must have its 8th row (pack_stem_weight)"
        self.lowp[name + ".w"] = lw

    def _add_conv(self, name: str, params, bias: bool):
        e = self.eng
        if name in self.frozen_bn:
            w_unfolded, scale = self.frozen_bn[name]
            self.master[name + ".w"] = pack_conv_weight(w_unfolded, torch.float32).to(e.device)
            self.row_scale[name + ".w"] = scale.detach().float().contiguous().to(e.device)
        else:
            self.master[name + ".w"] = pack_conv_weight(params[name + ".weight"], torch.float32).to(e.device)
        self.lowp[name + ".w"] = e.w[name + ".w"]
        if bias:
            self.master[name + ".b"] = e.w[name + ".b"]
        self.conv_names.append(name)

    def _refresh_derived(self):
        """Everything that is a function of the parameters and read by a kernel: backward-data weights, transposed fp32 heads,
        normalised prototypes."""
        e = self.eng
        wd = getattr(self, "wd", None)
        split = self.box_head == "split"
        if split and wd is not None:
            # the forward planes are read by the NEXT FORWARD: they are re-split on the main stream, behind the update
            ops.split_rows_bf16(self.master["fc1.w"], out=e.fc1_split)
            ops.split_rows_bf16(self.master["fc2.w"], out=e.fc2_split)
        if wd is None:  # first call: allocate the buffers (on the main stream); they are refilled in place every step (osr_pack_dgrad_weight)
            wd = {n: ops.pack_dgrad_weight(e.w[n + ".w"]) for n in self.conv_names}
            if split:  # the data gradients' operand: the bf16 planes of the transposed fp32 masters
                self.wt_split = {"fc1": ops.split_rows_bf16_t(self.master["fc1.w"]), "fc2": ops.split_rows_bf16_t(self.master["fc2.w"])}
            else:
                wd["fc1"] = ops.pack_dgrad_weight(e.fc1_w).view(e.fc1_w.shape[1], 1, 1, e.fc1_w.shape[0])
                wd["fc2"] = ops.pack_dgrad_weight(e.fc2_w).view(e.fc2_w.shape[1], 1, 1, e.fc2_w.shape[0])
            self.wd = wd
        else:  # every backward-data weight in one launch
            pairs = [(e.w[n + ".w"], wd[n]) for n in self.conv_names]
            if not split:
                pairs += [(e.fc1_w, wd["fc1"].view(e.fc1_w.shape[1], e.fc1_w.shape[0])), (e.fc2_w, wd["fc2"].view(e.fc2_w.shape[1], e.fc2_w.shape[0]))]
            sig = tuple(t.data_ptr() for pr in pairs for t in pr)
            if self._pack_plan is None or self._pack_plan[0] != sig:
                self._pack_plan = (sig, ops.pack_dgrad_multi_plan(pairs, self.device))
            # The backward-data weights are read by the NEXT BACKWARD only (the next forward reads the low-precision copies the update
            # kernel has just written): with the second stream in use the repack (0.15 ms, one launch) leaves the end of the iteration
            # -- it runs on that stream, idle until the next backward, behind the update, and the next backward waits for its event
            if self.side_wgrad and self._wside is not None and self.device.type == "cuda" and not torch.cuda.is_current_stream_capturing():
                self._wside.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self._wside):
                    ops.pack_dgrad_weight_multi_(self._pack_plan[1])
                    if split:
                        self._resplit_transposed()
                    self._pack_done = self._wside.record_event()
            else:
                ops.pack_dgrad_weight_multi_(self._pack_plan[1])
                if split:
                    self._resplit_transposed()
                self._pack_done = None
        self._refresh_heads()

    def _wait_pack(self) -> None:
        """The main stream waits for the repack behind the previous update (_refresh_derived runs it on the weight-gradient stream):
        before the backward reads the backward-data weights, and before the next update rewrites what the repack reads."""
        if getattr(self, "_pack_done", None) is not None:
            torch.cuda.current_stream(self.device).wait_event(self._pack_done)
            self._pack_done = None

    def _resplit_transposed(self) -> None:
        """box_head="split": the transposed bf16 planes of fc1.w / fc2.w (what the NEXT BACKWARD's data gradients read) from the
        updated fp32 masters, in place."""
        ops.split_rows_bf16_t(self.master["fc1.w"], out=self.wt_split["fc1"])
        ops.split_rows_bf16_t(self.master["fc2.w"], out=self.wt_split["fc2"])

    def _refresh_heads(self) -> None:
        """The derived tensors of the heads: transposed fp32 heads, normalised prototypes."""
        e = self.eng
        if not hasattr(self, "t_cls"):  # zero-padded transposes of the narrow fp32 heads: the padding rows are written once
            self.t_cls = torch.zeros((e.cls_w.shape[1], 32), dtype=torch.float32, device=e.device)    # (1024, 32): d rec = d logits(padded to 32) . W_cls
            self.t_pred = torch.zeros((e.pred_w.shape[1], 16), dtype=torch.float32, device=e.device)  # (1024, 16)
            self.t_dec = torch.empty((e.dec_w.shape[1], e.dec_w.shape[0]), dtype=torch.float32, device=e.device)  # (256, 1024): d emb = d rec . W_dec
            self.t_enc = torch.empty((e.enc_w.shape[1], e.enc_w.shape[0]), dtype=torch.float32, device=e.device)  # (1024, 256): d box_feats = d emb . W_enc
        self.t_cls[:, : e.cls_w.shape[0]].copy_(e.cls_w.t())
        self.t_pred[:, : e.pred_w.shape[0]].copy_(e.pred_w.t())
        ops.pack_dgrad_weight(e.dec_w, self.t_dec)
        ops.pack_dgrad_weight(e.enc_w, self.t_enc)
        e.protos = ops.l2_normalize_rows(self.master["protos"])

    # ---- forward with saved activations -------------------------------------------------------------------------
    def _forward(self, images, image_hw, hp, wp, gt_boxes, gt_classes, gt_count, keys, gt_masks=None):
        e = self.eng
        mask_kw = {} if gt_masks is None else dict(gt_masks=gt_masks, image_hw=image_hw)  # (the stock heads' mask branch)
        if e.ROI_LOSSES_NEED_IMAGE_HW:  # (the cascade clips the boxes it hands from stage to stage)
            mask_kw["image_hw"] = image_hw
        n = images.shape[0]
        s: dict = {}
        # anchor labels / sampling / targets depend on the ground truth only: a few small-grid launches (one workgroup per image)
        # that would otherwise sit in the stream between the RPN head and its loss; they run beside the backbone on a side stream
        cur = torch.cuda.current_stream(self.device)
        shapes = e.pyramid_shapes(hp, wp)
        lv = e._levels(shapes, n)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        if self.overlap_targets:
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                rpn_targets = e.rpn_targets_forward(lv, n, gt_boxes, gt_count, keys)
                targets_ready = self._side.record_event()
        out = self._forward_trunk(images, hp, wp, s)
        # RPN head, targets, losses
        keep: dict = {}
        sel = self._rpn_forward(out, image_hw, keep)
        s.update({k: keep[k] for k in self.RPN_SAVED}, sel=sel)
        self._proposal_status = sel["status_flags"]  # read with this iteration's overflow verdict (DynamicLossScale.record)
        assert list(keep["rpn_shapes"]) == list(shapes), "pyramid_shapes disagrees with the backbone"
        if self.overlap_targets:
            cur.wait_event(targets_ready)
            if not torch.cuda.is_current_stream_capturing():
                for t in rpn_targets.values():
                    t.record_stream(cur)
        else:
            rpn_targets = None
        rpn, rpn_state = e.rpn_losses_forward(sel, n, gt_boxes, gt_count, keys, targets=rpn_targets)
        s.update(rpn_state)
        # RoI heads on the sampled proposals
        roi, roi_state = e.roi_losses_forward(out, sel["boxes"], sel["scores"], sel["counts"], gt_boxes, gt_classes, gt_count, keys["roi"], **mask_kw)
        s.update(roi_state)
        # (_last_forward: what event_scalars() reads -- references only: nothing is computed or copied unless a logger asks)
        losses, self._last_forward = self._loss_dict(n, rpn, roi, sel, roi_state)
        return losses, s

    # what differs between the trainers in _forward (StandardRCNNTrainer replaces these three)
    RPN_SAVED = ("rpn_t", "rpn_shapes")  # what of the RPN head's `keep` the backward reads

    def _rpn_forward(self, feats, image_hw, keep: dict) -> dict:
        """CF-RPN head + proposal selection (un-fused when the dense backward wants the hidden state t of every anchor)."""
        self.eng.rpn_keep_hidden = not self.sparse_rpn_bwd
        return self.eng._rpn(feats, image_hw, keep, topk=self.eng.cfg["pre_nms_topk_train"])

    @staticmethod
    def _loss_dict(n, rpn, roi, sel, roi_state):
        """(the loss dict step() returns, _last_forward)"""
        losses = dict(loss_rpn_loc=rpn[0], loss_rpn_ctr=rpn[1], loss_box_reg=roi["loss_box_reg"], loss_iou=roi["loss_iou"],
                      loss_dml=roi["loss_dml"], loss_cls=roi["loss_cls"])
        return losses, dict(n=n, rpn_counts=rpn[2:6], prop_counts=sel["counts"], roi_counts=roi["roi_counts"], logits=roi_state["logits"],
                            cls_k=roi_state["cls_k"], nck=roi_state["nck"], batch_idx=roi_state["smp"]["batch_idx"])

    def _forward_trunk(self, images, hp, wp, s: dict) -> Dict[str, torch.Tensor]:
        """Backbone + FPN with the activations the backward reads saved into s (blocks, res, lat, p); returns p2..p6. This is the
        engine's own walk (_stem, _stages, _fpn) with `save`: which kernel a block gets is decided there, for inference and training."""
        e = self.eng
        pref, self._prefetched = self._prefetched, None
        if self.freeze_at == 0:
            # trainable stem: its output is kept for the backward (the fused stem + pool launch never writes it); same pooled bits
            x, xpad, stem = e._stem(images, hp, wp, keep_stem=True)
            frozen = {}
            s["stem"] = dict(xpad=xpad, s=stem, hp=hp, wp=wp)
        elif pref is not None and pref[0] is images and pref[1] == (hp, wp) and pref[4] == images._version:
            # the frozen prefix of THIS batch was computed under the previous iteration's backward (step(next_images=...)): take it
            x, frozen = pref[2]
            torch.cuda.current_stream(self.device).wait_event(pref[3])
        else:
            x, frozen = self._frozen_prefix(images, hp, wp)
        blocks: List[dict] = []  # (nothing of a frozen stage is needed by the backward)
        _, trained = e._stages(x, max(2, self.freeze_at + 1), 5, save=blocks, chain=self.chain_forward)
        s["blocks"], s["res"] = blocks, {**frozen, **trained}
        s["p"] = e._fpn(s["res"], save=s)
        return s["p"]

    def event_scalars(self) -> Dict[str, float]:
        """The ten scalars the reference puts into detectron2's EventStorage during a training iteration, for the LAST forward of this
        trainer (one small D2H copy; call it on logging iterations only):
          rpn/num_pos_anchors, rpn/num_neg_anchors, rpn/obj_num_pos_anchors, rpn/obj_num_neg_anchors (classification_free_rpn.py:459-463),
          rpn/num_proposals (:553-554), roi_head/num_fg_samples, roi_head/num_bg_samples (osrcnn_roi_heads.py:226-228: means over the
          images of the sampled foreground / background proposals), softmax_classifier/cls_accuracy, /fg_cls_accuracy, /false_negative
          (softmax_classifier.py:18-45 on the classifier's logits and the id-mapped targets; the last two only when a foreground row exists)."""
        lf = getattr(self, "_last_forward", None)
        if lf is None:
            return {}
        n, K = lf["n"], self.eng.cfg["num_known"]
        t = lf["cls_k"]
        if self.eng.id_map is None:  # VOC-COCO: known ids are 0..K-1 already, background = NUM_CLASSES -> K, every other class -> -1 (id_map, :224-229)
            t = torch.where(t < K, t, torch.where(t == lf["nck"], torch.full_like(t, K), torch.full_like(t, -1)))
        valid = lf["batch_idx"].view(-1) >= 0
        pred = lf["logits"][:, :K + 1].argmax(dim=1)
        fg = valid & (t >= 0) & (t < K)
        stats = torch.stack([valid.sum(), (valid & (pred == t)).sum(), fg.sum(), (fg & (pred == t)).sum(), (fg & (pred == K)).sum()]).to(torch.float32)
        host = torch.cat([lf["rpn_counts"].to(torch.float32).view(-1), lf["prop_counts"].to(torch.float32).view(-1), lf["roi_counts"].to(torch.float32).view(-1),
                          stats]).cpu().tolist()
        rc, pc, roi, st = host[:4], host[4:4 + n], host[4 + n:4 + n + 3 * n], host[4 + 4 * n:]
        out = {"rpn/num_pos_anchors": rc[0] / n, "rpn/num_neg_anchors": rc[1] / n, "rpn/obj_num_pos_anchors": rc[2] / n, "rpn/obj_num_neg_anchors": rc[3] / n,
               "rpn/num_proposals": sum(pc) / max(n, 1),
               "roi_head/num_fg_samples": sum(roi[1::3]) / n, "roi_head/num_bg_samples": sum(roi[2::3]) / n}
        if st[0] > 0:
            out["softmax_classifier/cls_accuracy"] = st[1] / st[0]
            if st[2] > 0:
                out["softmax_classifier/fg_cls_accuracy"] = st[3] / st[2]
                out["softmax_classifier/false_negative"] = st[4] / st[2]
        return out

    def _frozen_prefix(self, images, hp, wp):
        """Stem (+ preprocessing) and the frozen residual stages: what depends on the batch and on frozen weights only -- the output of
        the last frozen stage (the stem's max pool output when only the stem is frozen). freeze_at >= 1: the stem is frozen, nothing of
        it is needed by the backward, so the engine may run it as one launch."""
        x, _, _ = self.eng._stem(images, hp, wp)
        return self.eng._stages(x, 2, self.freeze_at)

    def _prefetch_frozen(self, images, hp, wp) -> None:
        """Software pipelining across iterations: the next batch's frozen prefix (a function of that batch and of weights no update
        touches) is enqueued on a stream of its own behind the main stream's CURRENT point -- called between the forward and the
        backward, it runs under the chain of small head / loss launches that leaves the GPU nearly idle there. The next step() that is
        handed the same tensor object picks the result up (and waits for it); any other batch recomputes. Same values either way."""
        if self.freeze_at < 1 or self.device.type != "cuda":  # (freeze_at 1: the prefix is the stem alone)
            return
        cur = torch.cuda.current_stream(self.device)
        if self._pre is None:
            self._pre = torch.cuda.Stream(device=self.device)
        self._pre.wait_event(cur.record_event())
        with torch.cuda.stream(self._pre):
            x, feats = self._frozen_prefix(images, hp, wp)
            done = self._pre.record_event()
        for t in [x] + list(feats.values()):
            t.record_stream(cur)
        images.record_stream(self._pre)  # (the caching allocator must not hand the batch's memory out while the side stream reads it)
        # Keyed on the tensor OBJECT and its version counter: a loader that refills one device buffer in place hands the same object with
        # a bumped version (recompute); next_images must not be written again before the step that consumes it. A new trainer
        # (load_state_dict drops the model's) starts without a prefetch (the prefix is a function of the frozen weights).
        self._prefetched = (images, (hp, wp), (x, feats), done, images._version)

    # ---- backward -------------------------------------------------------------------------------------------------
    def _f32_linear_bwd(self, x, dy, wt, name, dy_pad=None):
        """y = x W^T + b with fp32 operands on the exact-f32 GEMM: returns dx; writes dW, db. wt = W^T padded (k_in, n_pad)."""
        g = self.grad
        dyp = dy if dy_pad is None else torch.nn.functional.pad(dy, (0, dy_pad - dy.shape[1]))
        dx = ops.gemm_f32(dyp, wt, None)                                                    # (m, k_in)
        # dW / db only consume dy and the saved input: off the chain of small launches between the forward and the heavy backward, which
        # sits alone on the critical stream (the weight-gradient stream has nothing else to do at that point)
        self._wg(lambda: (ops.gemm_f32_tn(dy, x, out=g[name + ".w"]),                      # dW = dy^T x, (n_out, k_in)
                          ops.bias_grad(dy, g[name + ".b"])), dy, x)
        self._done(name + ".w", name + ".b")
        return dx

    def _done(self, *names: str) -> None:
        """The gradients of these parameters are final (their last launch is enqueued): a bucket they complete starts its
        all-reduce now, under the rest of the backward. The collective is issued from a stream of its own that waits for two
        EVENTS -- the main stream's and the weight-gradient stream's current points -- so it is ordered behind everything enqueued
        so far on both, and neither of the two compute streams waits for the other or for the collective (a wait_stream of the
        weight-gradient stream on the main one at every call re-serialised the two streams the single-GPU step gains 2 ms from)."""
        if not self._overlap:
            return
        ready = self.buckets.mark_ready(names)
        if not ready:
            return
        if self.device.type != "cuda":
            for b in ready:
                self.buckets.issue(b)
            return
        if self._cside is None:
            self._cside = torch.cuda.Stream(device=self.device)
        self._cside.wait_event(torch.cuda.current_stream(self.device).record_event())
        if self.side_wgrad and self._wside is not None:
            self._cside.wait_event(self._wside.record_event())
        with torch.cuda.stream(self._cside):
            for b in ready:
                self.buckets.issue(b)

    def _wg(self, fn, *reads: torch.Tensor, main: bool = False) -> None:
        """Run a weight / bias gradient launch group off the critical path: the chain of data gradients (dy of a layer -> dy of the
        layer below) stays on the main stream, the launches that only consume a layer's dy and its saved input (wgrad, its split
        reduction, the bias gradient) go to a second stream, where they fill the sparse last rounds of the data-gradient kernels
        and vice versa. `reads`: the tensors of the main stream the launches read (kept alive for the second stream)."""
        if not self.side_wgrad or main:
            fn()
            return
        cur = torch.cuda.current_stream(self.device)
        if self._wside is None:
            self._wside = torch.cuda.Stream(device=self.device)
        self._wside.wait_stream(cur)
        with torch.cuda.stream(self._wside):
            fn()
        if not torch.cuda.is_current_stream_capturing():
            for t in reads:
                t.record_stream(self._wside)

    def _backward_begin(self, grad_scale: float, overlap: bool) -> float:
        """What every backward does first; returns the factor its loss gradients carry (loss scale x grad_scale)."""
        S = self.loss_scale * grad_scale
        self._scale_used = self.loss_scale  # the update divides out the scale THIS backward multiplied in, whatever a poll does in between
        self._overlap = overlap and parallel.is_dist()
        self.buckets.reset()
        self._wait_pack()
        return S

    def _on_side(self, fn):
        """fn() on the weight-gradient stream behind the main stream's current point (main stream when side_wgrad is off)."""
        if not self.side_wgrad:
            return fn()
        cur0 = torch.cuda.current_stream(self.device)
        if self._wside is None:
            self._wside = torch.cuda.Stream(device=self.device)
        self._wside.wait_stream(cur0)
        with torch.cuda.stream(self._wside):
            return fn()

    def _join_side(self, ready, tensors) -> None:
        """The main stream waits for the event `ready` of _on_side's chain and adopts its tensors."""
        if self.side_wgrad:
            torch.cuda.current_stream(self.device).wait_event(ready)
            if not torch.cuda.is_current_stream_capturing():
                for t_ in tensors:
                    t_.record_stream(torch.cuda.current_stream(self.device))

    def _backward(self, s, n, grad_scale: float = 1.0, overlap: bool = True, prefetch=None):
        """Gradients of grad_scale * (sum of the six losses), times the loss scale, into self.grad. overlap: start each gradient
        bucket's all-reduce as soon as the backward has passed it (several ranks only; all_reduce_grads() then just waits)."""
        e, c, g = self.eng, self.eng.cfg, self.grad
        S = self._backward_begin(grad_scale, overlap)
        p = s["p"]
        # --- CF-RPN: losses -> tail -> weight gradient of the 3x3 conv (weights shared by the five levels). This chain depends on
        #     the forward only and meets the RoI heads' chain at the 3x3 conv's data gradient: it runs first, on the second stream,
        #     under the RoI heads' backward (whose RoIAlign scatter is bound by the atomic rate, not by the matrix cores) ---
        sel = s["sel"]
        rn = RPN_CONV

        def rpn_chain():
            lt_ = loss_types_of(c)
            d5 = ops.rpn_losses_bwd(sel["levels"], e.cell_anchors, n, sel["pred_deltas"], sel["pred_ctr"], s["labels"], s["obj_labels"], s["matched_boxes"],
                                    s["ctr_target"], c["rpn_loc_weight"], c["rpn_ctr_weight"], c["rpn_batch_size"], S, box_loss=lt_["rpn_box"],
                                    ctr_beta=lt_["rpn_ctr"][1])
            if self.sparse_rpn_bwd:
                # the loss touches the sampled anchors only: list the rows with a gradient, gather their im2col rows, and run the
                # head's backward on that list (csrc/osr_rpn_sparse.hip) -- hidden state recomputed, weight gradient and per-tap data
                # gradient as three small GEMMs; the dense launches spent 2 x 1.7 TFLOP on zeros
                cap = n * 2 * int(c["rpn_batch_size"])
                ids, rmap, cnt2 = ops.rpn_sparse_rows(d5, cap)
                # count2 = {listed, found}: rows beyond the cap are dropped by the list (the reference sampler bounds them by 2 x 256 per image;
                # another sampler, or NaN spilling into unsampled rows, could exceed it). The iteration's update is then skipped like a
                # gradient overflow, instead of applying an update that misses the coarsest levels' gradients -- on EVERY rank: the verdict
                # is rank-local (this rank's list), so it is folded into the gradient itself (an inf in this layer's bias gradient, below,
                # in front of its bucket's all-reduce) and reaches the other ranks through the sum; _update() then sees a non-finite
                # all-reduced buffer everywhere. (the flag used to gate this rank's update only; the peers applied theirs.)
                rows_fit = (cnt2[1:2] <= min(cap, self.sparse_rows_cap or cap)).to(torch.int32)
                cols, d5r = ops.rpn_gather_cols(sel["levels"], [p[k_] for k_ in PYRAMID], n, ids, d5)
                w3 = e.w[rn + ".w"].view(256, 9 * 256)
                t_rows = ops.linear(cols, w3, e.w[rn + ".b"], relu=True)
                dt_rows, dw_tail, db_tail = ops.cfrpn_tail_bwd(t_rows, e.rpn_wtail, d5r)
                g["rpn_tail.w"].copy_(dw_tail)
                g["rpn_tail.b"].copy_(db_tail)
                # (w3 is transposed inside every step here; StandardRCNNTrainer keeps a transposed copy refreshed with the parameters)
                y_rows = self._sparse_rpn_conv_bwd(cols, dt_rows, rows_fit, lambda: w3.t().contiguous())
                return (rmap, y_rows), torch.cuda.current_stream(self.device).record_event()
            dta, dw_tail, db_tail = ops.cfrpn_tail_bwd(s["rpn_t"], e.rpn_wtail, d5)
            g["rpn_tail.w"].copy_(dw_tail)
            g["rpn_tail.b"].copy_(db_tail)
            ready = torch.cuda.current_stream(self.device).record_event()
            off_ = 0
            for li_, (k_, (h_, w_)) in enumerate(zip(PYRAMID, s["rpn_shapes"])):
                rows_ = n * h_ * w_
                dtl_ = dta[off_:off_ + rows_].view(n, h_, w_, 256)
                off_ += rows_
                ops.conv2d_wgrad(p[k_], dtl_, 3, 3, 1, 1, dw=g[rn + ".w"], accumulate=li_ > 0)
                ops.bias_grad(dtl_, g[rn + ".b"], accumulate=li_ > 0)
            return (dta,), ready
        rpn_grad, rpn_ready = self._on_side(rpn_chain)
        self._done("rpn_tail.w", "rpn_tail.b", rn + ".w", rn + ".b")
        # --- RoI-head losses -> predictor / PLN / classifier (fp32 heads) ---
        lt = loss_types_of(c)
        d_pred = ops.roi_box_losses_bwd(s["pred"], s["boxes"], s["smp"]["gt_boxes"].view(-1, 4), s["cls"], s["ious"], c["num_classes"],
                                        c["bbox_reg_weights"], c["box_reg_weight"], c["iou_reg_weight"], S, box_loss=lt["roi_box"],
                                        iou_beta=lt["roi_iou"][1])
        d_logits = ops.softmax_ce_loss_bwd(s["logits"], s["cls_k"], s["nck"], c["cls_loss_weight"], S)
        d_emb_pln, d_protos = ops.pln_loss_bwd(s["emb"], self.master["protos"], s["cls_k"], s["ious"], c["pln_iou_threshold"], c["pln_alpha"],
                                               c["pln_beta"], c["pln_loss_weight"], S, reps=c["reps_per_class"], distance=c["pln_distance"])
        g["protos"].copy_(d_protos)
        self._done("protos")
        d_rec = self._f32_linear_bwd(s["rec"], d_logits, self.t_cls, "cls", dy_pad=32)
        d_emb = self._f32_linear_bwd(s["emb"], d_rec, self.t_dec, "dec")
        d_emb = ops.add_cast(d_emb, d_emb_pln, torch.float32)
        d_bf = self._f32_linear_bwd(s["box_feats"], d_emb, self.t_enc, "enc")
        d_bf2 = self._f32_linear_bwd(s["box_feats"], d_pred, self.t_pred, "pred", dy_pad=16)
        d_bf = ops.add_cast(d_bf, d_bf2, torch.float32)
        d_feat = self._box_head_bwd(s, d_bf, n)
        # --- CF-RPN 3x3 conv: data gradient per level, joined with the RoI heads' feature gradient (the chain above it ran on the
        #     second stream, see the top of this function) ---
        self._join_side(rpn_ready, rpn_grad)
        if self.sparse_rpn_bwd:
            dP = self._sparse_rpn_scatter(sel["levels"], s, n, rpn_grad, d_feat)
        else:
            dP, (dt_all,), off = {}, rpn_grad, 0
            roi_part = self._roi_share(d_feat) + [None]
            for li, (k, (h, w)) in enumerate(zip(PYRAMID, s["rpn_shapes"])):
                rows = n * h * w
                dP[k] = ops.conv2d_dgrad(dt_all[off:off + rows].view(n, h, w, 256), self.wd[rn], (h, w), 1, 1, add=roi_part[li])
                off += rows
        self._backward_trunk(s, dP, prefetch)

    def _sparse_rpn_conv_bwd(self, cols, dt_rows, rows_fit, w3_t) -> torch.Tensor:
        """The RPN head's 3x3 conv on the listed rows, behind the tail's backward: cols (cap, 2304) the gathered im2col rows, dt_rows
        (cap, 256) the hidden state's gradient -> weight gradient as a GEMM, bias gradient (poisoned unless the list fitted: rows_fit),
        and the per-tap data gradient y_rows (cap, 2304) fp32. w3_t: the (2304, 256) transposed weight matrix, or a callable that makes
        it (evaluated in front of the launch that reads it)."""
        g, cap = self.grad, cols.shape[0]
        ops.conv2d_wgrad(cols.view(1, cap, 1, 9 * 256), dt_rows.view(1, cap, 1, 256), 1, 1, dw=g[RPN_CONV + ".w"].view(256, 1, 1, 9 * 256))
        ops.bias_grad(dt_rows, g[RPN_CONV + ".b"])
        parallel.poison_unless_(rows_fit, g[RPN_CONV + ".b"].view(-1)[:1])
        return ops.linear(dt_rows, w3_t() if callable(w3_t) else w3_t, ops._zero_bias(9 * 256, self.device), out_dtype=torch.float32)

    def _roi_share(self, d_feat) -> List[torch.Tensor]:
        """The RoI heads' feature gradient of p2..p5 in the storage type."""
        return [(d if d.dtype == self.dtype else ops.add_cast(d, None, self.dtype)) for d in d_feat[:4]]

    def _sparse_rpn_scatter(self, levels, s, n, rpn_grad, d_feat) -> Dict[str, torch.Tensor]:
        """col2im of the listed anchors' per-tap gradients straight into the RoI heads' feature gradient (p6 has none: into zeros).
        levels: the level table of the pixel rows the list indexes. Returns dP (p2..p6)."""
        rmap, y_rows = rpn_grad
        h6, w6 = s["rpn_shapes"][4]
        glist = self._roi_share(d_feat) + [torch.zeros((n, h6, w6, 256), dtype=self.dtype, device=self.device)]
        ops.rpn_scatter_cols_add_(levels, n, rmap, y_rows, glist)
        return dict(zip(PYRAMID, glist))

    def _box_head_bwd(self, s, d_bf, n, fc=("fc1", "fc2"), pooled_grad_scale: float = 1.0, feat_f32: bool = False):
        """d box features (m,1024) fp32 -> FC2, FC1 (data + weight gradients) -> RoIAlign backward: the feature gradient per level.
        fc: the names of the two layers' masters and backward-data weights (a cascade has one pair per stage). pooled_grad_scale: a
        factor on the gradient that leaves the box head for RoIAlign ([d2] _ScaleGradient on the pooled features). feat_f32: the
        feature gradient in fp32 whatever the storage type (the caller sums several)."""
        c, g, dt = self.eng.cfg, self.grad, self.dtype
        fc1, fc2 = fc
        p = s["p"]
        if self.box_head_probe is not None:
            self.box_head_probe["d_bf"] = d_bf.clone()
        ops.relu_mask_(d_bf, s["box_feats"])
        m = d_bf.shape[0]
        if self.box_head == "split":
            # --- box head in fp32 operands: no cast of d_bf; FC2, FC1 on the split-precision kernels (the ReLU mask of h1 in the data
            #     gradient's epilogue), weight / bias gradients from the fp32 rows on the second stream ---
            d_h1 = ops.linear_split_dgrad(d_bf, self.wt_split[fc2], mask=s["h1"])
            self._wg(lambda: (ops.linear_split_wgrad(s["h1"], d_bf, dw=g[fc2 + ".w"]), ops.bias_grad(d_bf, g[fc2 + ".b"])), d_bf)
            self._done(fc2 + ".w", fc2 + ".b")
            pooled2 = s["pooled"].view(m, -1)
            d_pooled = ops.linear_split_dgrad(d_h1, self.wt_split[fc1])  # fp32: RoIAlign's backward sums it in fp32, _roi_share casts
            self._wg(lambda: (ops.linear_split_wgrad(pooled2, d_h1, dw=g[fc1 + ".w"]), ops.bias_grad(d_h1, g[fc1 + ".b"])), d_h1)
            self._done(fc1 + ".w", fc1 + ".b")
        else:
            dy2 = ops.add_cast(d_bf, None, dt)                                                  # (m,1024) low precision
            # --- box head: FC2, FC1 on the MFMA kernels ---
            d_h1 = ops.conv2d_dgrad(dy2.view(1, m, 1, -1), self.wd[fc2], (m, 1), mask=s["h1"].view(1, m, 1, -1)).view(m, -1)
            self._wg(lambda: (ops.conv2d_wgrad(s["h1"].view(1, m, 1, -1), dy2.view(1, m, 1, -1), 1, 1, dw=g[fc2 + ".w"].view(-1, 1, 1, g[fc2 + ".w"].shape[1])),
                              ops.bias_grad(dy2, g[fc2 + ".b"])), dy2)
            self._done(fc2 + ".w", fc2 + ".b")
            pooled2 = s["pooled"].view(1, m, 1, -1)
            d_pooled = ops.conv2d_dgrad(d_h1.view(1, m, 1, -1), self.wd[fc1], (m, 1))
            self._wg(lambda: (ops.conv2d_wgrad(pooled2, d_h1.view(1, m, 1, -1), 1, 1, dw=g[fc1 + ".w"].view(-1, 1, 1, g[fc1 + ".w"].shape[1])),
                              ops.bias_grad(d_h1, g[fc1 + ".b"])), d_h1)
            self._done(fc1 + ".w", fc1 + ".b")
        if pooled_grad_scale != 1.0:  # (behind the weight gradients' launches, which read d_h1, not d_pooled)
            d_pooled.mul_(pooled_grad_scale)
        if self.box_head_probe is not None:
            self.box_head_probe["d_pooled"] = d_pooled
        P = c["pooler_resolution"]
        shapes = [(p[k].shape[1], p[k].shape[2]) for k in PYRAMID[:4]]
        d_feat = ops.roi_align_bwd(d_pooled.view(m, P, P, -1), shapes, n, c["pooler_scales"], s["boxes"], s["smp"]["batch_idx"], c["canonical_level"],
                                   c["canonical_size"], 2, rois_per_image=m // n if m % n == 0 else None,  # (the sampled list is (n, S))
                                   out_dtype=dt if d_pooled.dtype == dt and not feat_f32 else None, aligned=c["pooler_aligned"],
                                   sampling_ratio=c["pooler_sampling_ratio"])
        if self.box_head_probe is not None:
            self.box_head_probe["d_feat"] = [d.clone() for d in d_feat]  # (the RPN's share is added into these tensors later)
        return d_feat

    def _backward_trunk(self, s, dP, prefetch) -> None:
        """dP (p2..p6 gradients, the heads' shares summed) -> p6 -> FPN -> res5 .. res3, weight gradients, the join of the streams."""
        g = self.grad
        p = s["p"]
        h5, w5 = p["p5"].shape[1], p["p5"].shape[2]
        dP["p5"] = ops.pool_bwd(dP["p6"], (h5, w5), dP["p5"], 1)  # p6 = p5[::2, ::2]
        # --- FPN: output convs, top-down adds, laterals (finest level first: its gradient flows up to the coarser sums) ---
        d_ls_prev = None
        d_res = {}
        for lvl in (2, 3, 4, 5):
            on, ln = f"backbone.fpn_output{lvl}", f"backbone.fpn_lateral{lvl}"
            ls = s["lat"][lvl]
            h, w = ls.shape[1], ls.shape[2]
            dpl = dP[f"p{lvl}"]
            up = ops.pool_bwd(d_ls_prev, (h, w), None, 0) if d_ls_prev is not None else None
            d_ls = ops.conv2d_dgrad(dpl, self.wd[on], (h, w), 1, 1, add=up)
            res = s["res"][f"res{lvl}"]
            self._wg(lambda ls=ls, dpl=dpl, res=res, d_ls=d_ls, on=on, ln=ln: (
                ops.conv2d_wgrad(ls, dpl, 3, 3, 1, 1, dw=g[on + ".w"]), ops.bias_grad(dpl, g[on + ".b"]),
                ops.conv2d_wgrad(res, d_ls, 1, 1, dw=g[ln + ".w"]), ops.bias_grad(d_ls, g[ln + ".b"])), dpl, d_ls)
            self._done(on + ".w", on + ".b", ln + ".w", ln + ".b")
            if lvl > self.freeze_at:
                d_res[lvl] = (d_ls, ln)  # the lateral's data gradient is formed together with the next stage's (see below)
            d_ls_prev = d_ls
        # --- backbone res5 -> res3: bottlenecks in reverse; G = gradient w.r.t. a block's output ---
        # G always arrives already masked by the ReLU that produced y (`post_mask=` of the launch that formed it): the join of
        # the two gradient branches and the ReLU below it are one epilogue (osr_conv2d_fwd_masked)
        G = None
        for bi in range(len(s["blocks"]) - 1, -1, -1):
            blk = s["blocks"][bi]
            pre, x, o1, o2, y, stride = blk["pre"], blk["x"], blk["o1"], blk["o2"], blk["y"], blk["stride"]
            s1, s2 = blk["s1"], blk["s2"]
            hy, wy = y.shape[1], y.shape[2]
            if blk["last_of_stage"]:  # the stage output also feeds its FPN lateral
                d_ls, ln = d_res[blk["stage"]]
                G = ops.conv2d_dgrad(d_ls, self.wd[ln], (hy, wy), 1, 0, add=G, post_mask=y)
            # (the last blocks of the backward: the weight-gradient stream is behind the data-gradient chain by then and nothing waits for
            # the chain's end, so their weight gradients ride on the main stream, beside the other stream's backlog)
            on_main = pre in self.wgrad_on_main
            d_o2 = ops.conv2d_dgrad(G, self.wd[pre + ".conv3"], (hy, wy), 1, 0, mask=o2)
            self._wg(lambda o2=o2, G=G, pre=pre: ops.conv2d_wgrad(o2, G, 1, 1, dw=g[pre + ".conv3.w"]), G, main=on_main)
            # (s2 == 2: osr_conv2d_dgrad_s2, the stride-2 3x3 layer's own data gradient)
            d_o1 = ops.conv2d_dgrad(d_o2, self.wd[pre + ".conv2"], (o1.shape[1], o1.shape[2]), s2, 1, mask=o1)
            self._wg(lambda o1=o1, d_o2=d_o2, x=x, d_o1=d_o1, pre=pre, s1=s1, s2=s2: (
                ops.conv2d_wgrad(o1, d_o2, 3, 3, s2, 1, dw=g[pre + ".conv2.w"]),
                ops.conv2d_wgrad(x, d_o1, 1, 1, s1, 0, dw=g[pre + ".conv1.w"])), d_o2, d_o1, main=on_main)
            if blk["first"]:
                self._wg(lambda x=x, G=G, pre=pre, stride=stride: ops.conv2d_wgrad(x, G, 1, 1, stride, 0, dw=g[pre + ".shortcut.w"]), G, main=on_main)
                self._done(pre + ".shortcut.w")
            self._done(pre + ".conv3.w", pre + ".conv2.w", pre + ".conv1.w")
            if blk["first"] and blk["stage"] == self.freeze_at + 1:
                break  # the block's input comes from frozen layers
            hx, wx = x.shape[1], x.shape[2]
            # x is the output of the block below (post-ReLU): its mask goes into the launch that completes G -- unless that block
            # is the last of its stage, whose G is completed (and masked) by the lateral's launch at the top of the next turn
            pm = None if bi > 0 and s["blocks"][bi - 1]["last_of_stage"] else x
            if blk["first"] and s1 != stride:
                # stride in conv2: conv1's share is dense, the shortcut's covers the even pixels only. The strided launch goes first
                # (into a zeroed dx), conv1's dense launch adds it and applies the mask: every pixel is summed and masked once
                dsc = ops.conv2d_dgrad(G, self.wd[pre + ".shortcut"], (hx, wx), stride, 0)
                G = ops.conv2d_dgrad(d_o1, self.wd[pre + ".conv1"], (hx, wx), 1, 0, add=dsc, post_mask=pm)
            elif blk["first"]:
                # (conv1's share is read back by the shortcut's launch at the strided pixels only: no zero fill of the others)
                dx = ops.conv2d_dgrad(d_o1, self.wd[pre + ".conv1"], (hx, wx), stride, 0, strided_only=stride > 1)
                G = ops.conv2d_dgrad(G, self.wd[pre + ".shortcut"], (hx, wx), stride, 0, add=dx, post_mask=pm)
            else:
                G = ops.conv2d_dgrad(d_o1, self.wd[pre + ".conv1"], (hx, wx), 1, 0, add=G, post_mask=pm)
        if self.freeze_at == 0:
            # G: the gradient of the pooled stem output (masked where it is <= 0 by the launch that formed it) -> max pool + ReLU
            # backward -> the stem's weight gradient (csrc/osr_stem_bwd.hip)
            st = s["stem"]
            ds = ops.stem_pool_bwd(st["s"], G)
            self._wg(lambda: ops.stem_wgrad(st["xpad"], ds, st["hp"], st["wp"], dw=g[STEM + ".w"]), ds, st["xpad"])
            self._done(STEM + ".w")
        if prefetch is not None:  # behind the last data gradient: the main stream is done, the weight-gradient stream still has its backlog
            self._prefetch_frozen(*prefetch)
        if self.side_wgrad and self._wside is not None:  # join: the update (and any collective issued from here on) sees every weight gradient
            torch.cuda.current_stream(self.device).wait_stream(self._wside)

    # ---- optimiser ------------------------------------------------------------------------------------------------
    def all_reduce_grads(self) -> int:
        """Sum the flat gradient buffer over the data-parallel ranks (RCCL over xGMI); returns the world size. The buckets whose
        parameters the backward has already marked are in flight since then (overlapped with the rest of the backward); this
        issues the remainder and waits for all of them."""
        return self.buckets.finish()

    def _update(self, world: int):
        """SGD on every master, gated on the device by the overflow flag: an iteration whose (all-reduced) gradients hold an inf or
        NaN changes neither parameters nor momentum (the reference trains in fp32 and cannot overflow; fp16 gradients can). The
        flag is read back lazily by `poll_overflow()` -- no host sync here."""
        gs = 1.0 / (getattr(self, "_scale_used", self.loss_scale) * world)
        self._apply_sgd(self.solver_options or SolverOptions(), self.lr, self.momentum, self.weight_decay, gs)
        self.scaler.record(self._ok, getattr(self, "_proposal_status", None))
        self._proposal_status = None

    def null_update(self) -> None:
        """The update's launches with nothing to apply (bench.py's no-collective timing): the caller has zeroed the gradient; learning
        rate 0, weight decay 0 and momentum factor 1 make p' = p - 0 * (1 * v + 0) and v' = 1 * v + 0 -- parameters, momentum buffers,
        low-precision copies and backward-data weights come out bit for bit as they went in, no verdict is queued in the loss scaler."""
        self._apply_sgd(SolverOptions(), 0.0, 1.0, 0.0, 1.0)

    def _param_rows(self) -> Dict[str, List[int]]:
        """Masters that hold several detectron2 parameters as contiguous row ranges: name -> row boundaries (see export_state_dict).
        Every other master is one parameter."""
        return {"rpn_tail.w": [0, 4, 5], "rpn_tail.b": [0, 4, 5],  # anchor_deltas, centerness
                "pred.w": [0, 4, 5], "pred.b": [0, 4, 5]}          # bbox_pred, iou_pred

    def _sgd_plan(self, o: SolverOptions, weight_decay: float):
        """The device-resident segment table of the update, built once per (bias lr factor, bias weight decay, weight decay, Nesterov)
        -- what the table itself carries -- and dropped when a buffer moves: one segment per detectron2 parameter (_param_rows), bias
        masters in the bias group."""
        sig = tuple(t.data_ptr() for k in self.master for t in (self.master[k], self.grad[k], self.mom[k]) + ((self.lowp[k],) if self.lowp.get(k) is not None else ()))
        if self._sgd_plans[0] != sig:
            self._sgd_plans = (sig, {})
        wd_bias = weight_decay if o.weight_decay_bias is None else o.weight_decay_bias
        key = (o.bias_lr_factor, wd_bias, weight_decay, o.nesterov)
        plans = self._sgd_plans[1]
        if key not in plans:
            rows = self._param_rows()
            entries = []
            for k, pm in self.master.items():
                bias = k.endswith(".b")
                bounds = rows.get(k, [0, pm.shape[0]])
                for r0, r1 in zip(bounds[:-1], bounds[1:]):
                    entries.append((pm, self.grad[k], self.mom[k], self.row_scale.get(k), self.lowp.get(k), r0, r1,
                                    o.bias_lr_factor if bias else 1.0, wd_bias if bias else weight_decay, o.nesterov))
            plans[key] = ops.sgd_segment_plan(entries, self.device)
        return plans[key]

    def _apply_sgd(self, o: SolverOptions, lr: float, momentum: float, weight_decay: float, gs: float) -> None:
        """Every master in ONE launch (osr_sgd_step_multi_ex over the segment table), then every backward-data weight in one more
        (_refresh_derived). The [d2] solver options o: per-parameter clipping of the averaged gradient grad * gs * row_scale, the bias
        group, Nesterov momentum; the neutral SolverOptions() is torch.optim.SGD's plain step. The overflow flag is cleared by
        osr_check_finite over the flat buffer, or, with norm clipping, by the norm pass (osr_grad_norm_partials covers every master:
        the flat buffer's alignment padding is never written). Runs after all_reduce_grads(), so every rank computes the same
        coefficients."""
        self._wait_pack()  # (two updates without a backward in between: the previous repack still reads the copies this one rewrites)
        self._ok.fill_(1)
        if o.clip != "norm":  # (in front of the plan lookup: the host's walk over the buffers' addresses then runs under this launch)
            ops.check_finite_(self.grad_flat, self._ok)
        plan = self._sgd_plan(o, weight_decay)
        if o.clip == "norm":
            ops.grad_norm_partials_(plan, gs, o.norm_type, self._ok)
        ops.sgd_step_multi_ex_(plan, lr, momentum, gs, o.clip, o.clip_value, o.norm_type, self._ok)
        self._refresh_derived()

    # several ranks: step k applies the verdicts of the updates up to k - 1 - MULTI_RANK_LAG, waited for -- the same set on every rank
    # (they are functions of the all-reduced gradient), so the scales cannot drift apart, and the host still runs two iterations ahead
    # of the GPU (waiting for update k - 1 at the top of step k exposed the ~150 small update launches and the next forward's launch
    # latency on every iteration)
    MULTI_RANK_LAG = 2

    def poll_overflow(self, wait: bool = False, lag: int = 0) -> bool:
        """Drain, IN ORDER, the verdicts of the updates that have finished (wait=True: of every update issued so far). True when
        at least one of them was skipped because of non-finite gradients. Dynamic loss scaling as GradScaler does it: an
        overflow halves the scale (floor 1.0) and counts in `overflow_steps`; `scale_growth_interval` consecutive clean updates
        double it again, never past the configured scale. Every update has a pinned slot of its own, so a verdict is never lost
        however far the host runs ahead. With several ranks step() calls this with wait=True and lag=MULTI_RANK_LAG: every rank then applies the same
        verdicts (they are functions of the all-reduced gradient) at the same iteration, and the scales cannot drift apart.
        (`wait=True` is also what the checkpoint writer uses, so that no skipped or half-applied state is written blind.)"""
        return self.scaler.poll(wait, lag)

    def step(self, images, image_hw, hp, wp, gt_boxes, gt_classes, gt_count, keys, update: bool = True, next_images=None,
             gt_masks=None) -> Dict[str, torch.Tensor]:
        """One iteration: returns the loss dict (GPU scalars). update=False leaves the parameters untouched (gradients stay in
        self.grad, scaled by loss_scale). next_images (optional): the NEXT iteration's image batch, if the loader already has it: its
        frozen prefix (stem + frozen stages) is computed under this iteration's backward (_prefetch_frozen) and used by the next
        step() that is given that same tensor. gt_masks: (n, gmax, Hm, Wm) uint8 bitmask planes, for a trainer whose heads have a mask
        branch (StandardRCNNTrainer with MODEL.MASK_ON)."""
        # earlier iterations' verdicts adjust the loss scale here, at one deterministic point of the iteration; with several ranks
        # the call waits for them, so that all ranks change the scale at the same iteration (see poll_overflow)
        self.poll_overflow(wait=parallel.is_dist(), lag=self.MULTI_RANK_LAG if parallel.is_dist() else 0)
        losses, saved = self._forward(images, image_hw, hp, wp, gt_boxes, gt_classes, gt_count, keys, **({} if gt_masks is None else {"gt_masks": gt_masks}))
        # the data-gradient chain shares the GPU with the weight-gradient stream: tell the conv tile model (osr_conv_params.concurrency; a
        # tile-selection hint only -- results do not depend on it) so that it may take the 256 x 256 tile where a lone stream would not
        with ops.concurrent_streams(self.backward_concurrency_hint):
            self._backward(saved, images.shape[0], overlap=update, prefetch=(next_images, hp, wp) if next_images is not None else None)
        if update:
            self._update(self.all_reduce_grads())
        return losses

    def export_optimizer_state(self) -> Dict[str, torch.Tensor]:
        """Momentum buffers (CPU copies) for a checkpoint that is resumed exactly ([d2] checkpoints carry the optimizer state)."""
        out = {k: v.detach().cpu().clone() for k, v in self.mom.items()}
        # One rank: every issued update's verdict goes into the scale that is written. Several ranks: the queue is left ALONE -- the ranks apply
        # verdicts in lockstep inside step() (MULTI_RANK_LAG), and a drain here, on whichever ranks happen to write a checkpoint, would change
        # one rank's scale 2-3 steps before its peers' (different scales multiplied into the same all-reduce). A collective checkpoint
        # writer that wants the newest verdicts in the file calls poll_overflow(wait=True) on EVERY rank first (run_net.save_checkpoint).
        if not parallel.is_dist():
            self.poll_overflow(wait=True)
        out[self.SCALE_KEY] = torch.tensor([self.scaler.scale, float(self.scaler.clean_steps), float(self.scaler.overflow_steps), self.scaler.scale_max],
                                           dtype=torch.float64)
        return out

    SCALE_KEY = "__dynamic_loss_scale__"  # (scale, consecutive clean updates, skipped updates so far, configured scale)

    def load_optimizer_state(self, state: Dict[str, torch.Tensor]) -> None:
        state = dict(state)
        sc = state.pop(self.SCALE_KEY, None)
        if sc is not None:  # a run that had backed off resumes at the scale it was written with, not at the configured one
            self.scaler.scale, self.scaler.clean_steps, self.scaler.overflow_steps = float(sc[0]), int(sc[1]), int(sc[2])
        for k, v in state.items():
            if k not in self.mom or tuple(self.mom[k].shape) != tuple(v.shape):
                raise KeyError(f"optimizer state {k}: not a momentum buffer of this trainer")
            self.mom[k].copy_(v.to(self.mom[k].device))

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters under detectron2 names and layouts (un-folded conv weights), for load_state_dict /
        checkpointing ([d2] DetectionCheckpointer writes these keys under "model")."""
        out = self._export_trunk()
        t_w, t_b = self.master["rpn_tail.w"].cpu(), self.master["rpn_tail.b"].cpu()
        out["proposal_generator.rpn_head.anchor_deltas.weight"] = t_w[:4].reshape(4, -1, 1, 1).clone()
        out["proposal_generator.rpn_head.anchor_deltas.bias"] = t_b[:4].clone()
        out["proposal_generator.rpn_head.centerness.weight"] = t_w[4:5].reshape(1, -1, 1, 1).clone()
        out["proposal_generator.rpn_head.centerness.bias"] = t_b[4:5].clone()
        p_w, p_b = self.master["pred.w"].cpu(), self.master["pred.b"].cpu()
        out["roi_heads.box_predictor.bbox_pred.weight"], out["roi_heads.box_predictor.bbox_pred.bias"] = p_w[:4].clone(), p_b[:4].clone()
        out["roi_heads.box_predictor.iou_pred.weight"], out["roi_heads.box_predictor.iou_pred.bias"] = p_w[4:5].clone(), p_b[4:5].clone()
        for short, long in (("enc", "roi_heads.dml.encoder"), ("dec", "roi_heads.dml.decoder"), ("cls", "roi_heads.softmaxcls.cls_score")):
            out[long + ".weight"], out[long + ".bias"] = self.master[short + ".w"].cpu().clone(), self.master[short + ".b"].cpu().clone()
        out["roi_heads.dml.representatives"] = self.master["protos"].cpu().clone()
        return out

    def _export_trunk(self) -> Dict[str, torch.Tensor]:
        """Backbone / FPN / RPN 3x3 conv and box head FC1 / FC2 masters under detectron2 names and layouts."""
        out: Dict[str, torch.Tensor] = {}
        if STEM + ".w" in self.master:  # stem view (64, 8, 1, 32) -> (64, 3, 7, 7)
            out[STEM + ".weight"] = self.master[STEM + ".w"].view(64, 8, 8, 4)[:, :7, :7, :3].permute(0, 3, 1, 2).contiguous().cpu()
        for n in self.conv_names:
            out[n + ".weight"] = self.master[n + ".w"].permute(0, 3, 1, 2).contiguous().cpu()
            if n + ".b" in self.master:
                out[n + ".bias"] = self.master[n + ".b"].cpu().clone()
        self._export_box_heads(out)
        return out

    def _export_box_heads(self, out: Dict[str, torch.Tensor]) -> None:
        self._export_box_head(out, "fc1", "fc2", "roi_heads.box_head.")

    def _export_box_head(self, out: Dict[str, torch.Tensor], fc1_name: str, fc2_name: str, prefix: str) -> None:
        pr = self.eng.cfg["pooler_resolution"]
        fc1 = self.master[fc1_name + ".w"]  # (out, ph, pw, c) flattened -> the reference's (out, c*ph*pw)
        out[prefix + "fc1.weight"] = fc1.view(fc1.shape[0], pr, pr, -1).permute(0, 3, 1, 2).reshape(fc1.shape[0], -1).contiguous().cpu()
        out[prefix + "fc1.bias"] = self.master[fc1_name + ".b"].cpu().clone()
        out[prefix + "fc2.weight"] = self.master[fc2_name + ".w"].cpu().clone()
        out[prefix + "fc2.bias"] = self.master[fc2_name + ".b"].cpu().clone()
