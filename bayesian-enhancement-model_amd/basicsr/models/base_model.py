"""Model wrapper base (basicsr/models/base_model.py): device placement, checkpoint saving / loading (:236-343), training-state
save / resume (:345-394), schedulers (:124-168), learning-rate update with linear warm-up (:209-230), loss-dict reduction (:396-421).
File formats are the reference's: ``<label>_<iter>.pth`` = {param_key: state_dict on CPU}, ``<iter>.state`` = {epoch, iter,
optimizers: [state_dict], schedulers: [state_dict], best_metric, ...}; both load with ``torch.load(weights_only=True)``.

Also what ImageEnhancer and ConditionGenerator repeat line for line in the reference (image_enhancer_model.py /
condition_generator_model.py): net_g built, placed and loaded (:31-63 / :32-75), the optimizer (:103-131 / :115-144), the averaged net
(:69-83 / :81-95), the step's tail -- clip, optimizer step, model_ema (:204-214 / :208-218) --, the averaged net in validation
(:239-247 / :240-248), ``save`` (:340-350 / :346-356) and ``save_best`` (:352-382 / :358-388).  A model class gives ``_build_net()``
and keeps what differs."""
import contextlib
import glob
import os
import time
from collections import OrderedDict

import torch

from basicsr.models import lr_scheduler
from bem.train import BemAdam, BemAdamW, WeightEma


class _LazyLog(OrderedDict):
    """log_dict whose values are device scalars until somebody reads them (the reference calls .item() inside the step, one host
    synchronisation per iteration; here the step stays asynchronous and the read pays it)."""

    def __getitem__(self, k):
        v = super().__getitem__(k)
        if torch.is_tensor(v):
            v = float(v.mean().item())
            super().__setitem__(k, v)
        return v

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class BaseModel:
    def __init__(self, opt):
        self.opt = opt
        self.device = torch.device("cuda" if opt.get("num_gpu", 1) != 0 and torch.cuda.is_available() else "cpu")
        self.is_train = opt.get("is_train", False)
        self.schedulers, self.optimizers = [], []
        self.log_dict = OrderedDict()

    def model_to_device(self, net):
        return net.to(self.device)

    def sync_gradients(self, optimizer):
        """opt['dist']: average the gradients over the ranks before clipping (what the reference gets from DistributedDataParallel,
        base_model.py:97-100); without an initialised process group a distributed option file is an error, not N silent replicas."""
        if not self.opt.get("dist"):
            return
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            raise RuntimeError("opt['dist'] is set but torch.distributed is not initialised (launch with --launcher pytorch)")
        optimizer.all_reduce_grads()

    def get_bare_model(self, net):
        return net.module if hasattr(net, "module") else net

    # -- net_g and its averaged copy --------------------------------------------------------------------------------
    def _build_net(self):
        """A fresh net of this model on the host (net_g, and net_g_ema where one is kept)."""
        raise NotImplementedError

    def _init_net_g(self):
        """net_g on the device with ``path.pretrain_network_g`` loaded; in training the refusals of what the f32 HIP path does not offer,
        then the class's ``init_training_settings``."""
        opt, name = self.opt, type(self).__name__
        self.net_g = self.model_to_device(self._build_net())
        path = opt["path"].get("pretrain_network_g")
        if path is not None:
            self.load_network(self.net_g, path, opt["path"].get("strict_load_g", True), opt["path"].get("param_key", "params"))
        self.mask = None
        if self.is_train:
            if opt.get("use_amp"):
                raise NotImplementedError(f"{name}: use_amp is not available on the f32 HIP path")
            if opt["train"].get("mixing_augs", {}).get("mixup", False):
                raise NotImplementedError(f"{name}: mixup augmentation is host-side data preparation outside the hot path")
            self.init_training_settings()

    def load_network(self, net, load_path, strict=True, param_key="params"):
        ck = torch.load(load_path, map_location="cpu", weights_only=True)
        if param_key is not None and param_key not in ck and "params" in ck:
            print(f"Loading: {param_key} does not exist, use params.", flush=True)       # base_model.py:331-335
            param_key = "params"
        sd = ck[param_key] if param_key is not None and param_key in ck else ck
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        net.load_state_dict(sd, strict=strict)

    def init_ema_weights(self, net_ema, weight_ema):
        """The averaged net's start (image_enhancer_model.py:77-83): ``params_ema`` of ``path.pretrain_network_g`` where that is set (a
        resumed run restores both copies; a file without the key gives ``params``), else a copy of net_g.  It stays in eval()."""
        path = self.opt["path"].get("pretrain_network_g")
        if path is not None:
            self.load_network(net_ema, path, self.opt["path"].get("strict_load_g", True), "params_ema")     # copies into the flat buffer's views
        else:
            weight_ema.copy_from_net()
        net_ema.eval()

    def cpu_state_dict(self, net):
        """The bare net's state dict on the CPU, a wrapper's ``module.`` prefix stripped: what a checkpoint file holds under its key."""
        return OrderedDict((k[7:] if k.startswith("module.") else k, v.detach().cpu()) for k, v in self.get_bare_model(net).state_dict().items())

    def with_ema_state(self, save_dict):
        """``save_dict`` plus ``params_ema`` when the model keeps an averaged net: save_best's file then also holds the weights that
        earned the metric."""
        if hasattr(self, "net_g_ema"):
            save_dict["params_ema"] = self.cpu_state_dict(self.net_g_ema)
        return save_dict

    def save(self, epoch, current_iter, **kwargs):
        """``net_g_<iter>.pth`` (with ``params_ema`` where an averaged net is kept) and the training state."""
        if hasattr(self, "net_g_ema"):
            self.save_network([self.net_g, self.net_g_ema], "net_g", current_iter, param_key=["params", "params_ema"])
        else:
            self.save_network(self.net_g, "net_g", current_iter)
        self.save_training_state(epoch, current_iter, **kwargs)

    def save_best(self, best_metric, param_key="params"):
        """``<experiments_root>/best_psnr_<psnr>_<iter>.pth``, replacing any earlier best_* file."""
        if self.opt.get("rank", 0) != 0:
            return None
        root = self.opt["path"]["experiments_root"]
        path = os.path.join(root, f"best_psnr_{best_metric['psnr']:.2f}_{best_metric['iter']}.pth")
        if not os.path.exists(path):
            for f in glob.glob(f"{root}/best_*"):
                os.remove(f)
            os.makedirs(root, exist_ok=True)
            torch.save(self.with_ema_state({param_key: self.cpu_state_dict(self.net_g)}), path)
        return path

    def save_network(self, net, net_label, current_iter, param_key="params"):
        """``<models>/<net_label>_<iter>.pth`` (iter -1 -> 'latest'); net / param_key may be lists of equal length (base_model.py:236-280)."""
        if self.opt.get("rank", 0) != 0:                       # @master_only in the reference (base_model.py:235)
            return None
        it = "latest" if current_iter == -1 else current_iter
        save_path = os.path.join(self.opt["path"]["models"], f"{net_label}_{it}.pth")
        nets = net if isinstance(net, list) else [net]
        keys = param_key if isinstance(param_key, list) else [param_key]
        assert len(nets) == len(keys), "The lengths of net and param_key should be the same."
        save_dict = {k: self.cpu_state_dict(n) for n, k in zip(nets, keys)}
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        retry, err = 3, None
        while retry > 0:                                       # "avoid occasional writing errors" (:265-278)
            try:
                torch.save(save_dict, save_path)
                return save_path
            except OSError as e:
                err = e
                time.sleep(1)
            retry -= 1
        raise IOError(f"Cannot save {save_path}.") from err

    def save_training_state(self, epoch, current_iter, **kwargs):
        """``<training_states>/<iter>.state`` with every optimizer's and scheduler's state_dict (base_model.py:345-376); rank 0 only."""
        if self.opt.get("rank", 0) != 0 or current_iter == -1:
            return None
        state = {"epoch": epoch, "iter": current_iter, "optimizers": [], "schedulers": []}
        state.update(kwargs)
        state["optimizers"] = [o.state_dict() for o in self.optimizers]
        state["schedulers"] = [s.state_dict() for s in self.schedulers]
        state["best_metric"] = kwargs["best_metric"]           # the reference requires it (:370)
        save_path = os.path.join(self.opt["path"]["training_states"], f"{current_iter}.state")
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        torch.save(state, save_path)
        return save_path

    def resume_training(self, resume_state):
        """Reload optimizers and schedulers (base_model.py:379-394)."""
        ro, rs = resume_state["optimizers"], resume_state["schedulers"]
        assert len(ro) == len(self.optimizers), "Wrong lengths of optimizers"
        assert len(rs) == len(self.schedulers), "Wrong lengths of schedulers"
        for o, sd in zip(self.optimizers, ro):
            o.load_state_dict(sd)
        for s, sd in zip(self.schedulers, rs):
            s.load_state_dict(sd)

    # -- training-side helpers -------------------------------------------------------------------------------------
    def setup_optimizers(self):
        normal, custom = [], []
        for k, v in self.net_g.named_parameters():
            if v.requires_grad:
                (custom if "impfusion" in k else normal).append(v)
        groups = [{"params": normal, "lr_mult": 1, "name": "normal_params"},
                  {"params": custom, "lr_mult": 1, "decay_mult": 0, "name": "custom_params"}]
        cfg = dict(self.opt["train"]["optim_g"])
        kind = cfg.pop("type")
        if kind not in ("Adam", "AdamW"):                                             # image_enhancer_model.py:124-130
            raise NotImplementedError(f"optimizer {kind} is not supperted yet.")
        self.optimizer_g = (BemAdamW if kind == "AdamW" else BemAdam)(groups, **cfg)
        self.optimizers.append(self.optimizer_g)

    def init_optimizer_and_ema(self):
        """The end of ``init_training_settings``: optimizer, schedulers and -- with ``train.ema_decay > 0`` -- the averaged net, built like
        net_g; it is only validated and saved, on every rank the same average of the same parameters (never wrapped)."""
        self.ema_decay = self.opt["train"].get("ema_decay", 0)
        self.optimizers, self.schedulers = [], []
        self.setup_optimizers()
        self.setup_schedulers()
        self.weight_ema = None
        if self.ema_decay > 0:
            print(f"Use Exponential Moving Average with decay: {self.ema_decay}", flush=True)
            self.net_g_ema = self._build_net().to(self.device)
            self.weight_ema = WeightEma(self.optimizer_g, self.get_bare_model(self.net_g), self.net_g_ema)
            self.init_ema_weights(self.net_g_ema, self.weight_ema)

    def finish_step(self, skip=(), state=None):
        """After backward(): gradients averaged over the ranks, global-norm clip, AdamW (``skip``: parameters outside this iteration's
        graph; ``state``: the bem.train.StepState of a step that is being captured) and model_ema(decay) as one more launch behind it.
        Returns the gradient norm as a device scalar."""
        self.sync_gradients(self.optimizer_g)
        mgn = self.opt["train"].get("max_grad_norm")
        total_norm = self.optimizer_g.clip_grad_norm_(mgn if mgn else float("inf"))
        if state is not None:
            self.optimizer_g.step_captured(state, skip=skip)
        else:
            self.optimizer_g.step(skip=skip)
        if self.weight_ema is not None:
            self.weight_ema.update(self.ema_decay)
        return total_norm

    @staticmethod
    def unweighted(loss, weight):
        """A loss term as it is logged: without its weight."""
        return loss.detach() if weight == 1 else loss.detach() / weight

    @contextlib.contextmanager
    def validated_net(self):
        """The net a validation runs -- the averaged one where there is one -- in eval() mode, put back into train() afterwards."""
        net = self.net_g_ema if hasattr(self, "net_g_ema") else self.net_g
        was_training = net.training
        net.eval()
        try:
            yield net
        finally:
            if was_training:
                net.train()

    def report_validation(self, head, sums, count):
        """metric_results = the means of ``sums`` ({'psnr': sum over the images, ...}) and the rank-0 line behind ``head``; returns the
        mean PSNR."""
        self.metric_results = {k: v / max(count, 1) for k, v in sums.items()}
        if self.opt.get("rank", 0) == 0:
            print(f"{head},\t\t # " + "\t # ".join(f"{k}: {v:.4f}" for k, v in self.metric_results.items()), flush=True)
        return self.metric_results["psnr"]

    def setup_schedulers(self):
        sch = dict(self.opt["train"]["scheduler"])
        kind = sch.pop("type")
        total = self.opt["train"].get("total_iter")                 # LinearLR / VibrateLR take it alone, not the block's keys (:151-158)
        build = {"MultiStepLR": lambda o: lr_scheduler.MultiStepRestartLR(o, **sch),
                 "MultiStepRestartLR": lambda o: lr_scheduler.MultiStepRestartLR(o, **sch),
                 "CosineAnnealingRestartLR": lambda o: lr_scheduler.CosineAnnealingRestartLR(o, **sch),
                 "CosineAnnealingRestartCyclicLR": lambda o: lr_scheduler.CosineAnnealingRestartCyclicLR(o, **sch),
                 "TrueCosineAnnealingLR": lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, **sch),
                 "LinearLR": lambda o: lr_scheduler.LinearLR(o, total),
                 "VibrateLR": lambda o: lr_scheduler.VibrateLR(o, total)}.get(kind)
        if build is None:           # CosineAnnealingWarmupRestarts / CosineAnnealingLRWithRestart included: the reference's file lacks them too
            raise NotImplementedError(f"Scheduler {kind} is not implemented yet.")
        for o in self.optimizers:
            self.schedulers.append(build(o))

    def _get_init_lr(self):
        return [[g["initial_lr"] for g in o.param_groups] for o in self.optimizers]

    def _set_lr(self, lr_groups_l):
        for o, lrs in zip(self.optimizers, lr_groups_l):
            for g, lr in zip(o.param_groups, lrs):
                g["lr"] = lr

    def update_learning_rate(self, current_iter, warmup_iter=-1):
        if current_iter > 1:
            for s in self.schedulers:
                s.step()
        if current_iter < warmup_iter:
            self._set_lr([[v / warmup_iter * current_iter for v in g] for g in self._get_init_lr()])

    def get_current_learning_rate(self):
        return [g["lr"] for g in self.optimizers[0].param_groups]

    def get_current_log(self):
        return self.log_dict

    def reduce_loss_dict(self, loss_dict):
        """Average over ranks when distributed (one reduce of the stacked scalars to rank 0, base_model.py:405-415)."""
        with torch.no_grad():
            if self.opt.get("dist"):
                keys = list(loss_dict)
                losses = torch.stack([loss_dict[k].reshape(()) for k in keys], 0)
                torch.distributed.reduce(losses, dst=0)
                if self.opt.get("rank", 0) == 0:
                    losses /= self.opt["world_size"]
                loss_dict = {k: v for k, v in zip(keys, losses)}
            return _LazyLog((k, v.detach()) for k, v in loss_dict.items())
