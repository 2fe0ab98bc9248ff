"""ConditionGenerator (basicsr/models/condition_generator_model.py): Stage-I net + BNN conversion (:32-75), the losses of the training
settings (:77-113), data feed (:148-174), the training step with the KL term (:176-218), validation (:272-334).  What it shares with
ImageEnhancer -- loading, optimizer, the averaged net ``net_g_ema`` (converted like net_g), the step's tail, checkpoints -- is BaseModel's."""
import os
from collections import OrderedDict

import torch

from basicsr.archs import build_network
from basicsr.bayesian import convert2bnn, convert2bnn_selective, get_kl_loss, set_prediction_type
from basicsr.losses import build_loss
from basicsr.models.base_model import BaseModel
from basicsr.utils.registry import MODEL_REGISTRY
from bem import autograd as ag
from bem import bayes, ops
from bem.train import StepState


@MODEL_REGISTRY.register()
class ConditionGenerator(BaseModel):
    def __init__(self, opt):
        super().__init__(opt)
        self._init_net_g()

    def _build_net(self):
        net = build_network(self.opt["network_g"])
        cfg = {"sigma_init": self.opt.get("sigma_init", 0.05), "decay": 0.998, "pretrain": False}
        (convert2bnn_selective if self.opt.get("selective", True) else convert2bnn)(net, cfg)
        return net

    def init_training_settings(self):
        self.net_g.train()
        train_opt = self.opt["train"]
        self.cri_pix = build_loss(train_opt["pixel_opt"]).to(self.device) if train_opt.get("pixel_opt") else None
        if train_opt.get("perceptual_opt"):
            raise NotImplementedError("ConditionGenerator: perceptual_opt is not available for Stage I: its predictions are 8x8 planes, below what "
                                      "VGG19's deeper layers (conv5_4 needs 16x16) can take, and its training step is a captured graph; "
                                      "remove `perceptual_opt` (the Stage-I option files of the reference train on the pixel loss)")
        if train_opt.get("ssim_opt"):
            raise NotImplementedError("ConditionGenerator: ssim_opt is not available for Stage I: its predictions are 8x8 planes, smaller than "
                                      "the 11x11 window of SSIMLoss; remove `ssim_opt` (the Stage-I option files of the reference train on the "
                                      "pixel loss)")
        if train_opt.get("lpips_opt"):
            raise NotImplementedError("ConditionGenerator: lpips_opt is not available for Stage I: its predictions are 8x8 planes, below the "
                                      "31x31 that LPIPSLoss's AlexNet trunk needs; remove `lpips_opt` (the Stage-I option files of the "
                                      "reference train on the pixel loss)")
        if train_opt.get("combined_opt"):
            raise NotImplementedError("ConditionGenerator: combined_opt is not available for Stage I: its predictions are 8x8 planes, smaller than "
                                      "the 11x11 window of CombinedLoss's SSIM part and below what its VGG19 trunk can take; remove "
                                      "`combined_opt` (the Stage-I option files of the reference train on the pixel loss)")
        self.cri_perceptual = None
        if self.cri_pix is None:
            raise ValueError("Both pixel and perceptual losses are None.")
        self.init_optimizer_and_ema()

    def feed_train_data(self, data):
        kind = self.opt["condition"]["type"]
        if kind == "mean":
            self.lq = data["lq_down"].to(self.device)
            if "gt" in data:
                self.gt = data["gt_down"].to(self.device)
        elif kind == "histogram":
            self.lq = data["hist_lq"].to(self.device)
            if "gt" in data:
                self.gt = data["hist_gt"].to(self.device)
        self.mask = data["mask"].to(self.device) if "mask" in data else None

    def feed_data(self, data):
        kind = self.opt["condition"]["type"]
        if kind not in ("mean", "histogram"):
            raise NotImplementedError(f"{kind} is not supported yet.")
        self.feed_train_data({k: v for k, v in data.items() if k != "mask"})

    def optimize_parameters(self, current_iter):
        """zero_grad -> net_g(lq, mask) (mask dropped after the first scheduler period) -> l_total = 0.01 * l_kl / mini_batch + l_pix ->
        backward -> clip_grad_norm_ -> AdamW (:176-218).  The train.png dumps every 100 iterations are host-side logging, not done here.

        The step is ~2000 launches on 8x8 .. 2x2 planes, i.e. launch-bound: after one ordinary run per input geometry it is captured into a
        HIP graph and replayed, with everything that differs between iterations read from device memory
        (bem.train.StepState).  BEM_STAGE1_GRAPH=0, injected eps, a distributed run or an active launch profile keep the ordinary form."""
        periods = self.opt["train"]["scheduler"].get("periods")       # a scheduler without periods has no first period: the mask stays
        if periods and current_iter > periods[0]:
            self.mask = None
        skip = [self.net_g.mask_token] if self.mask is None else []
        if (os.environ.get("BEM_STAGE1_GRAPH", "1") != "0" and bayes.scope.ctx is None and not self.opt.get("dist") and ops._PROF is None
                and self.optimizer_g.graph_safe(skip)):
            return self._optimize_graphed(current_iter, skip)
        return self._step_body(current_iter, skip, None)

    def _step_body(self, current_iter, skip, state):
        self.optimizer_g.zero_grad()
        # the weight draws of iteration i come from Philox streams keyed by (manual_seed, rank, i): a resumed run draws what the
        # uninterrupted run would have drawn (the reference's resumed run restarts torch's generator instead)
        seed, rank = int(self.opt.get("manual_seed") or 0) & 0xFFFFFFFF, int(self.opt.get("rank", 0))
        if state is not None:
            ctx = bayes.SampleCtx(1, None, seed=seed, rank=rank, epoch_dev=state.epoch_dev)
        else:
            ctx = bayes.scope.ctx or bayes.SampleCtx(1, None, seed=seed, rank=rank, epoch=int(current_iter) & 0xFFFFFF)   # an enclosing context (injected eps) wins
        with bayes.sampling(ctx):
            _, preds = self.net_g(self.lq.contiguous(), mask=self.mask)
        loss_dict = OrderedDict()
        l_kl = get_kl_loss(self.net_g)
        loss_dict["l_kl"] = l_kl.detach()
        l_pix = self.cri_pix(preds, self.gt)
        loss_dict["l_pix"] = self.unweighted(l_pix, self.opt["train"]["pixel_opt"].get("loss_weight", 1))
        l_total = ag.ScaledSumFn.apply(l_pix, l_kl, 0.01 / self.opt["datasets"]["train"]["mini_batch_sizes"][0])
        l_total.backward()
        # a parameter outside this iteration's graph has .grad None in the reference and is skipped by AdamW: the mask token without a mask
        # model_ema(decay) (:213-214) after the step has put skipped slices back: the mask token is averaged in every iteration.  decay is
        # constant, so a captured step records the launch with it by value, as one more node on the same stream
        total_norm = self.finish_step(skip, state)
        if state is not None:
            return loss_dict, total_norm              # reduced once per replay, outside the captured body
        self.log_dict = self.reduce_loss_dict(loss_dict)
        return total_norm

    def _optimize_graphed(self, current_iter, skip):
        """One captured step per input geometry: {"graph", "state", static inputs, the step's loss tensors}.  The first iteration with a
        geometry runs the ordinary way (it is also the warm-up that leaves every lazily created buffer in place); the second records the
        step -- recording launches nothing -- and is then replayed like all later ones."""
        key = (tuple(self.lq.shape), tuple(self.gt.shape), None if self.mask is None else tuple(self.mask.shape))
        graphs = self.__dict__.setdefault("_graphs", {})
        g = graphs.get(key)
        bank_sig = lambda: getattr(bayes.BayesBank.of(self.get_bare_model(self.net_g)), "sig", None)
        if isinstance(g, dict) and g["bank_sig"] is not bank_sig():
            g = None                 # the bank rebuilt its tables (a parameter / gradient / prior buffer moved): the recorded launches point at the old ones
        if g is None:
            graphs[key] = "warm"
            return self._step_body(current_iter, skip, None)
        if g == "warm":
            g = {"state": StepState(self.lq.device), "lq": self.lq.clone(), "gt": self.gt.clone(),
                 "mask": None if self.mask is None else self.mask.clone(), "graph": torch.cuda.CUDAGraph()}
            feed = self.lq, self.gt, self.mask
            self.lq, self.gt, self.mask = g["lq"], g["gt"], g["mask"]
            torch.cuda.synchronize()
            try:
                with bayes.capturing(g["state"]), torch.cuda.graph(g["graph"]):
                    g["losses"], g["norm"] = self._step_body(current_iter, skip, g["state"])
            finally:
                self.lq, self.gt, self.mask = feed
            g["bank_sig"] = bank_sig()
            graphs[key] = g
        for dst, src in ((g["lq"], self.lq), (g["gt"], self.gt), (g["mask"], self.mask)):
            if dst is not None and dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        g["state"].upload(current_iter)
        g["graph"].replay()
        g["state"].advance()
        self.log_dict = self.reduce_loss_dict(g["losses"])
        return g["norm"]

    # -- validation (:236-334) ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def validation(self, dataloader, current_iter, tb_logger=None, save_img=False, rgb2bgr=True, use_image=True):
        """Mean PSNR of the predicted condition planes against the down-sampled ground truth, deterministic weights (mu), float form on
        the device."""
        tot, cnt = 0.0, 0
        with self.validated_net() as net:                             # :239-247: the averaged net where there is one
            set_prediction_type(net, True)
            for data in dataloader:
                self.feed_data(data)
                pred = net(self.lq.contiguous())[-1]
                h, w = pred.shape[-2:]
                _, ps = ops.candidate_finalize(pred.contiguous(), self.gt.contiguous(), 1, h, w, False)
                tot += float(ps.sum())
                cnt += pred.shape[0]
            set_prediction_type(net, False)
        return self.report_validation("Validation", {"psnr": tot}, cnt)
