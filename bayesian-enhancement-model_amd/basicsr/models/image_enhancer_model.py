"""ImageEnhancer (basicsr/models/image_enhancer_model.py): Stage-II net wrapper -- the net (:31-63) and the training step
(:65-101 losses, :133-148 feed_train_data, :165-216 optimize_parameters), validation (:265-328).  What it shares with ConditionGenerator
-- loading, optimizer, the averaged net, the step's tail, checkpoints -- is BaseModel's.

The step runs entirely on the HIP path: condition upsample + concat (bem.ops), forward / backward (bem.autograd), global-norm clip +
AdamW on one flat buffer (bem.train.BemAdamW), the pixel loss and -- with ``train.perceptual_opt`` -- the VGG19 perceptual loss
(bem.percep) and -- with ``train.ssim_opt`` -- the SSIM term of basicsr/losses/my_loss.py:37-38 (csrc/ssim_loss.hip) and -- with
``train.lpips_opt`` -- the LPIPS term (bem.lpips, csrc/lpips.hip) and -- with ``train.combined_opt`` -- the six-term recipe of
basicsr/losses/my_loss.py:51-74 (basicsr.losses.CombinedLoss, csrc/pixstat_loss.hip), with no host synchronisation inside ``optimize_parameters`` -- loss values and the
gradient norm come back as device scalars (read them when logging).  AMP (`use_amp`) is not offered: the path is f32.
``train.ema_decay > 0`` keeps ``net_g_ema`` (BaseModel), which is validated instead of net_g (:239-247)."""
from collections import OrderedDict

import torch

from basicsr.archs import build_network
from basicsr.losses import build_loss
from basicsr.models.base_model import BaseModel
from basicsr.utils.registry import MODEL_REGISTRY
from bem import autograd as ag
from bem import ops
from bem.archs import AttnDrop, attn_drop_stream_id

_ALL_NONE = "Pixel, perceptual, SSIM, LPIPS and combined losses are all None."


@MODEL_REGISTRY.register()
class ImageEnhancer(BaseModel):
    def __init__(self, opt):
        super().__init__(opt)
        self.mixing_flag = False
        self._init_net_g()

    def _build_net(self):
        return build_network(self.opt["network_g"])

    # ---------------------------------------------------------------------------------------------------------------
    def init_training_settings(self):
        train_opt = self.opt["train"]
        if train_opt.get("use_amp"):
            raise NotImplementedError("ImageEnhancer: use_amp is not available on the f32 HIP path")
        self.net_g.train()
        self.cri_pix = build_loss(train_opt["pixel_opt"]).to(self.device) if train_opt.get("pixel_opt") else None
        self.cri_perceptual = build_loss(train_opt["perceptual_opt"]).to(self.device) if train_opt.get("perceptual_opt") else None
        self.cri_ssim = build_loss(train_opt["ssim_opt"]).to(self.device) if train_opt.get("ssim_opt") else None
        self.cri_lpips = build_loss(train_opt["lpips_opt"]).to(self.device) if train_opt.get("lpips_opt") else None
        if train_opt.get("combined_opt"):                              # without the block the model has no such attribute
            self.cri_combined = build_loss(train_opt["combined_opt"]).to(self.device)
        if self.cri_pix is None and self.cri_perceptual is None and self.cri_ssim is None and self.cri_lpips is None and not hasattr(self, "cri_combined"):
            raise ValueError(_ALL_NONE)
        self._ssim_metrics()                                           # a val.metrics entry validation would refuse is refused now
        self.init_optimizer_and_ema()

    def feed_train_data(self, data):
        dev = self.device
        self.lq = data["lq"].to(dev)
        self.gt = data["gt"].to(dev) if "gt" in data else None
        self.mask = data["mask"].to(dev) if "mask" in data else None
        cond = self.opt["condition"]
        if cond["type"] == "histogram":
            raise NotImplementedError("condition type 'histogram' is not used by the shipped option files")
        gd = data["gt_down"].to(dev).contiguous()
        nl = cond.get("noise_level", 0)
        # conds = gt_down + randn_like(gt_down) * noise_level  (:143-148); the draw comes from the device Philox stream in the reserved
        # condition-noise key space (bit 62, as BEMPipeline.candidates): unique per rank and per iteration, so replicas never share a draw
        # and a resumed run continues the sequence instead of replaying it
        it = int(getattr(self, "current_iter_hint", 0)) or (getattr(self, "_cond_calls", 0) + 1)
        self._cond_calls = it
        key = (1 << 62) | (int(self.opt.get("rank", 0)) << 44) | (it & ((1 << 44) - 1))
        self.conds = ops.add(gd, ops.randn(tuple(gd.shape), dev, int(self.opt.get("manual_seed", 0) or 0), key), nl) if nl else gd

    feed_data = feed_train_data

    def _net_input(self):
        """cat(lq, F.interpolate(conds, scale_factor=s, 'bilinear')) as one 6-channel tensor, written in place by two launches."""
        s = self.opt["condition"].get("scale_down", 0) + self.opt["condition"].get("hist_patch_size", 0)
        B, _, H, W = self.lq.shape
        x = torch.empty(B, 6, H, W, device=self.lq.device, dtype=torch.float32)
        ops.copy_channels(self.lq.contiguous(), x, 0)
        ops.bilinear_up(self.conds, s, dst=x, dst_c0=3)
        return x

    attn_drop_masks = None      # parity runs: the keep flags of the next step's decomposition calls, one (B,2,32,32) tensor per call

    def _attn_drop(self, current_iter):
        """The frozen decomposition's attention dropout (QD model3, live in train() mode) draws from the device Philox stream in a key space
        of its own (bem.archs.attn_drop_stream_id: bit 61), a function of (manual_seed, rank, iteration) with the iteration feed_train_data
        derived: replicas never share a draw and a resumed run continues the sequence.  Returns the decomposition, or None without one."""
        dec = getattr(self.get_bare_model(self.net_g), "decomp", None)
        if dec is None or not dec.cross_attn.p > 0:
            return None
        it = int(getattr(self, "_cond_calls", 0) or current_iter)
        dec.attn_drop = AttnDrop(int(self.opt.get("manual_seed", 0) or 0), attn_drop_stream_id(int(self.opt.get("rank", 0)), it), self.attn_drop_masks)
        return dec

    def optimize_parameters(self, current_iter):
        self.optimizer_g.zero_grad()
        x = self._net_input()
        dec = self._attn_drop(current_iter)
        try:
            _, preds = self.net_g(x, mask=None)                       # the Decomp* archs ignore the MIM mask (DDWavelet_arch.py:301)
        finally:
            if dec is not None:
                dec.attn_drop = None                                  # the record is this forward's alone
        loss_dict = OrderedDict()
        # :183-191: l_total = l_pix + l_percep (+ l_ssim, my_loss.py:37-38, + l_lpips, + l_comb, my_loss.py:51-74) over the configured terms; preds feeds each of them,
        # its gradients are summed by bem_add_f32 (ag.fork_n; one term alone takes preds itself)
        crits = (self.cri_pix, self.cri_perceptual, self.cri_ssim, self.cri_lpips, getattr(self, "cri_combined", None))
        heads = iter(ag.fork_n(preds, sum(c is not None for c in crits)))
        l_pix, l_percep, l_ssim, l_lpips, l_comb = ((None if c is None else c(next(heads), self.gt)) for c in crits)
        if l_percep is not None:
            l_percep, _ = l_percep                                       # None with perceptual_weight <= 0 (:186): the term is off
        l_total = None
        for l in (l_pix, l_percep, l_ssim, l_lpips, l_comb):
            if l is not None:
                l_total = l if l_total is None else ag.AddFn.apply(l_total, l)
        if l_total is None:
            raise ValueError(_ALL_NONE)
        if l_pix is not None:
            loss_dict["l_pix"] = self.unweighted(l_pix, self.opt["train"]["pixel_opt"].get("loss_weight", 1))
        if l_percep is not None:
            loss_dict["l_percep"] = l_percep.detach() / self.cri_perceptual.perceptual_weight          # :188
        if l_ssim is not None:
            loss_dict["l_ssim"] = self.unweighted(l_ssim, self.cri_ssim.loss_weight)                    # 1 - SSIM
        if l_lpips is not None:
            loss_dict["l_lpips"] = self.unweighted(l_lpips, self.cri_lpips.loss_weight)                 # the mean distance
        if l_comb is not None:
            loss_dict["l_comb"] = self.unweighted(l_comb, self.cri_combined.loss_weight)                # the recipe's own sum
            for name, v in self.cri_combined.parts.items():                                            # its active parts, unweighted
                loss_dict["l_comb_" + name] = v
        l_total.backward()
        total_norm = self.finish_step()
        self.log_dict = self.reduce_loss_dict(loss_dict)
        return total_norm

    # -- validation (image_enhancer_model.py:259-325) -------------------------------------------------------------------------
    @torch.no_grad()
    def validation(self, dataloader, current_iter, tb_logger=None, save_img=False, rgb2bgr=True, use_image=True):
        """Mean PSNR of net_g over a validation loader, conditions derived from the ground truth as in training (feed_data: gt_down +
        noise).  The inference kernels run the forward; PSNR is the float form ``10 log10(1 / mse)`` on [0,1] tensors computed on the
        device (the reference's ``use_image: false`` branch; its uint8 / cv2 image branch and image dumps are host-side reporting)."""
        ssim_names = self._ssim_metrics()
        tot, cnt, ssim_tot = 0.0, 0, 0.0
        with self.validated_net() as net:                             # :239-247: the averaged net where there is one
            for data in dataloader:
                self.feed_train_data(data)
                B, _, H, W = self.lq.shape
                pred = net(self._net_input())[-1]
                h, w = data.get("crop_hw", (H, W))
                gt = self.gt[..., :h, :w].contiguous()
                _, ps = ops.candidate_finalize(pred.contiguous(), gt, 1, h, w, False)
                tot += float(ps.sum())
                cnt += B
                if ssim_names and ssim_tot == ssim_tot:
                    if h <= 10 or w <= 10:
                        if self.opt.get("rank", 0) == 0:
                            print(f"Warning: validation SSIM needs images larger than its 11x11 window, got {h} x {w}: reported as nan", flush=True)
                        ssim_tot = float("nan")
                    else:
                        # calculate_ssim (basicsr/metrics/psnr_ssim.py:88-132) on tensor2img values of the cropped output and target
                        ssim_tot += float(ops.ssim(pred[..., :h, :w].contiguous(), gt, 1).sum())
        return self.report_validation(f"Validation {getattr(dataloader.dataset, 'opt', {}).get('name', 'val')}",
                                      {"psnr": tot, **{name: ssim_tot for name in ssim_names}}, cnt)

    def _ssim_metrics(self):
        """Names of the ``val.metrics`` entries of type calculate_ssim.  crop_border / test_y_channel on one of them are refused: the device
        metric (bem_ssim_f32) is the whole-image RGB form, which is what every option file of the reference asks for (0 / false)."""
        names = []
        for name, m in ((self.opt.get("val") or {}).get("metrics") or {}).items():
            if not isinstance(m, dict) or m.get("type") != "calculate_ssim":
                continue
            if m.get("crop_border", 0) != 0 or m.get("test_y_channel", False):
                raise NotImplementedError(f"ImageEnhancer: val.metrics.{name}: crop_border={m.get('crop_border', 0)}, test_y_channel="
                                          f"{m.get('test_y_channel', False)}: validation SSIM is computed on the whole RGB image (crop_border 0, "
                                          "test_y_channel false)")
            if name == "psnr":
                raise ValueError("ImageEnhancer: val.metrics.psnr is the PSNR entry's result; give the calculate_ssim entry another name")
            names.append(name)
        return names
