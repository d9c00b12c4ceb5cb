"""Drop-in mirror of the reference's ``src.litmodule`` (VLBLitModule / VLBLitModuleConfig).

Same class names, the same 16 config fields, the same hooks with the same meaning
(src/litmodule/videollama2_vlb_litmodule.py:126-379): ``configure_model``, ``make_weight_mask``,
``forward(x_video, x_lang, weight_mask, attention_mask)`` -> ``(regression_output, l2_reg)``,
``training_step(batch)`` -> scalar loss (no batch_idx), ``validation_step(batch)`` ->
``{'loss','brain_preds','brain_vals'}``, ``configure_optimizers()`` -> ``([opt],[{scheduler...}])``,
``self.log("train/brain_loss", ...)``.  Module attribute names ``nnmodule``, ``hrf_layer``,
``ridge_layer``, ``layer_norm1``, ``layer_norm2``, ``dropout`` are kept.

What differs, on purpose: all arithmetic runs in libvlb HIP kernels; the backward pass is explicit
(``training_step`` leaves fp32 gradients in ``param.grad`` of the trainable masters and returns the
loss), because there is no autograd graph through hand-written kernels.
"""
from __future__ import annotations

import contextlib
import math
import os
import warnings
from dataclasses import dataclass

import torch

from . import ops
from .backbone import Backbone, Weights, destack_decoder_layer
from .geometry import Geometry, geometry_7b, geometry_mini
from .head import HEAD_PARAMS, LAYER_MIX, BrainHead, check_loss, check_readout_layers, check_subjects, target_weight_levels
from .optim import FULLFT_EMA_MESSAGE, VlbAdamW
from .optim_groups import assign_groups, group_specs, normalize_optimizer_groups


def _lightning():
    """``lightning.pytorch`` when it is importable, else None (this container and the GPU boxes: absent)."""
    try:
        import lightning.pytorch as lp
        return lp
    except Exception:
        return None


_LP = _lightning()

if _LP is not None:
    class _Base(_LP.LightningModule):
        """Real Lightning is installed: VLBLitModule IS a ``LightningModule`` (reference litmodule :160), so the reference's
        unchanged ``train.py:41-56`` can hand it to ``lightning.pytorch.Trainer.fit``.  The kernels have no autograd graph;
        the bridge to Lightning's automatic optimisation is ``_ExplicitLoss`` below (``loss.backward()`` hands out the
        gradients ``training_step`` already computed) plus the hooks ``configure_gradient_clipping`` (the YAML's
        ``gradient_clip_val: 1`` is applied inside the fused AdamW kernel), ``transfer_batch_to_device`` and
        ``state_dict`` on VLBLitModule."""

        def __init__(self):
            super().__init__()
            self.logged: dict[str, float] = {}

        def log(self, name, value, **kw):
            self.logged[name] = value
            tr = getattr(self, "_trainer", None)
            if tr is not None and isinstance(tr, _LP.Trainer):       # the built-in runner reads self.logged instead
                super().log(name, value, **kw)
else:
    class _Base:
        """The slice of ``lightning.pytorch.LightningModule`` the reference's module uses (``self.log``, ``self.device``,
        train/eval mode, ``self.trainer``) for environments without Lightning; ``train.py`` then runs the built-in
        ``phantom_vlb_amd.trainer.Trainer`` (same YAML keys).  With Lightning installed the class above is used instead."""

        def __init__(self):
            self.training = True
            self.logged: dict[str, float] = {}
            self.trainer = None

        def log(self, name, value, **kw):
            self.logged[name] = value

        def train(self, mode: bool = True):
            self.training = mode
            return self

        def eval(self):
            return self.train(False)


class _ExplicitLoss(torch.autograd.Function):
    """The scalar ``training_step`` returns: the loss value the kernels computed, attached to the trainable Parameters so that
    Lightning's automatic optimisation can call ``loss.backward()``.  The backward pass ran explicitly inside
    ``training_step`` (hand-written kernels, no autograd tape); ``backward`` here only (re-)attaches those gradient buffers as
    the Parameters' ``.grad`` - Lightning zeroes the gradients between ``training_step`` and ``backward`` - and returns no
    autograd gradients, so nothing is accumulated twice.  Under ``accumulate_grad_batches = k > 1`` Lightning calls
    ``(loss / k).backward()``: the module has already applied the 1/k (``training_step`` scales the head backward, the
    gradients never flow through autograd), so the upstream gradient must be exactly that 1/k - anything else (a loss
    scaler, a different divisor) would silently give a differently scaled step and raises instead.  The check reads one
    scalar back and runs for k > 1 only; at k = 1 the upstream gradient is taken to be 1, as before."""

    @staticmethod
    def forward(ctx, loss, module, *params):
        ctx.module = module
        ctx.n = len(params)
        ctx.k = module.accumulate_grad_batches
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, gout):
        if ctx.k > 1:
            got, want = float(gout), 1.0 / ctx.k
            if abs(got - want) > 1e-6 * want:
                raise ValueError(f"loss.backward() arrived with an upstream gradient of {got!r}, expected 1/accumulate_grad_batches = "
                                 f"{want!r}: the module scales its explicit backward by 1/k itself, so the loss must be divided by "
                                 f"k = {ctx.k} and by nothing else (no loss scaling)")
        ctx.module._attach_gradients()
        return (None, None) + (None,) * ctx.n


def check_accumulate_grad_batches(k) -> int:
    """``accumulate_grad_batches`` as both runners accept it: an int >= 1."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"accumulate_grad_batches={k!r}: an integer >= 1 is needed (1 = one optimiser step per batch)")
    return k


class _LinearInfo:
    """Stand-in for an ``nn.Linear`` leaf when a weight store lists its module tree (``Backbone.named_modules``)."""
    is_linear = True

    def __init__(self, out_features, in_features):
        self.out_features, self.in_features = out_features, in_features


def find_all_linear_names(model):
    """reference :36-55 (from VideoLLaMA2's trainer): leaf names of every linear layer outside the multimodal
    modules, minus ``lm_head`` - the LoRA ``target_modules``.  ``model`` is anything with ``named_modules()``:
    a torch module tree (``nn.Linear`` leaves) or this package's ``Backbone`` (leaves listed from its weights)."""
    lora_module_names = set()
    multimodal_keywords = ["mm_projector", "vision_tower", "vision_resampler"]
    for name, module in model.named_modules():
        if any(k in name for k in multimodal_keywords):
            continue
        if isinstance(module, torch.nn.Linear) or getattr(module, "is_linear", False):
            names = name.split(".")
            lora_module_names.add(names[0] if len(names) == 1 else names[-1])
    lora_module_names.discard("lm_head")
    return sorted(lora_module_names)


@dataclass
class VLBLitModuleConfig:
    """Field for field the reference's dataclass (src/litmodule/...:138-153) plus optional extras."""
    model_path: str
    freeze_backbone: bool
    use_lora: bool
    lora_r: int | None
    lora_alpha: int | None
    lora_dropout: float | None
    dropout_rate: float
    num_target: int
    l2_lambda: float
    lr: float
    betas: list[float]
    eps: float
    weight_decay: float
    lr_scheduler_name: str
    last_epoch: int
    t_max: int
    # ---- extras (not in the reference; all optional)
    geometry: str = "7b"            # "7b" | "mini"
    init_seed: int = 1234
    gradient_clip_val: float = 1.0  # the Trainer's gradient_clip_val, applied inside the fused AdamW
    pack_tokens: bool = True        # drop each clip's padded tail rows (flash-attn varlen equivalent)
    fp8_gemm: bool = False          # full fine-tune only: decoder forward / dgrad GEMMs on the MX-fp8 MFMA path (configs[4])
    cache_features: bool = False    # frozen backbone only: keep each clip's pooled features, later epochs run the head alone
    feature_cache_dir: str | None = None    # persist the feature caches there (feature_cache.py; loaded on a matching fingerprint)
    merge_lora_for_eval: bool = False   # LoRA only: eval-mode forwards run the frozen-path decoder on merged weights (LoraState.merge)
    loss: str = "mse"               # "mse" (reference :302) | "cosine" (its docstring's alternative, :290-301) | "pearson"; + l2 always
    # decoder layers the head reads (HF hidden_states[k], k in [1, L] or [-L, -1]; more than one: a learned softmax mix of their
    # pooled features, ``layer_mix.weight``); the decoder stops at the highest.  None: hidden_states[-1], as the reference
    readout_layers: list[int] | None = None
    # two or more subject names: one backbone (and adapter set), one ridge head per subject (``ridge_layer.linear.weight``
    # [G,V,E]); every batch then carries "subject" (datamodule.config.subjects, the same list).  None: one head, as the reference
    subjects: list[str] | None = None
    # "closed_form": once the train split's feature cache is complete, ridge_layer.linear.{weight,bias} are set to the exact
    # minimiser of the mse objective for the current LN parameters (dropout not included), fp64 on the device;
    # training then goes on as configured.  None: AdamW finds them, as the reference
    ridge_fit: str | None = None
    # ridge_fit="closed_form" only.  A list of two or more distinct positive values: the fit chooses l2_lambda among them by
    # blocked K-fold cross-validation on the train split (held-out Pearson r, from the same one pass over the cache; DESIGN
    # §5.3.6), solves with it and keeps it for every later step (the configured l2_lambda holds until then and need not be
    # in the list).  A clip's fold is (its rank in its head's clips // ridge_cv_block) % ridge_cv_folds.  None: l2_lambda as given
    ridge_lambda_grid: list[float] | None = None
    ridge_cv_folds: int = 5
    ridge_cv_block: int = 128           # contiguous clips per block, about three minutes of TRs: a choice, not a measurement
    # ridge_lambda_grid only.  True: the same cross-validation chooses one grid point per (head, target), each row of the ridge
    # weight is solved with its own l2_lambda and every later step's penalty is sum_v lambda_v ||W_v||^2;
    # head.l2_lambda keeps the one global choice, for reporting.  False: one l2_lambda for the whole head
    ridge_lambda_per_target: bool = False
    # ridge_fit="closed_form" only.  True: the fit and its cross-validation accept ``target_weights`` / ``set_target_weights``
    # and minimise the weighted objective of DESIGN §5.3.8 in closed form (§5.3.9): masked targets (weight 0, NaN allowed in
    # the data) reach no sum and get W_v = 0, b_v = 0; a head may hold at most 8 distinct positive weights (one factorisation
    # each).  Without weights it changes nothing.  False: weights and the closed-form fit refuse each other
    ridge_fit_weighted: bool = False
    # learning rate / weight decay per group of trainables: up to 7 entries {params: [fnmatch pattern, ...],
    # lr_scale: float = 1.0, weight_decay: float | None = None} over the names trainable_named_parameters() yields; the first
    # entry with a matching pattern takes a tensor, what no entry matches keeps lr / weight_decay; lr_scale multiplies lr (the
    # scheduler then drives every group), weight_decay None = the configured one.  None: one group, as the reference (:357-363)
    optimizer_groups: list[dict] | None = None
    # exponential moving average of the trainables, kept inside the fused AdamW launch: 0 < ema_decay < 1, the
    # decay of the average (0.999 is usual); LoRA and frozen-backbone runs, one process.  None: no average, nothing changes
    ema_decay: float | None = None
    ema_warmup: bool = True             # the t-th update's decay is min(ema_decay, (1 + t) / (10 + t)); False: ema_decay from the first
    ema_eval: bool = True               # validation and the merged export read the averaged weights (VLBLitModule.averaged_weights)
    # path of a .npy file of per-target loss weights: [num_target], or [G, num_target] with ``subjects`` (one row
    # per subject, in that order); with ``subjects`` the path may hold the literal ``{subject}`` instead and name one
    # [num_target] file per subject.  Finite, >= 0; a 0/1 file is a mask (targets with weight 0 are neither trained on nor
    # scored, and may be NaN in the data).  None: every target counts alike, as the reference
    target_weights: str | None = None
    # the evaluation pass (test_step / Trainer.test): per-target r, R^2 and mse over a held-out split.
    # score_block: contiguous clips per bootstrap block (a clip's block is its rank in its head's clips // score_block, the rule
    # of ridge_cv_block); score_bootstrap: resamples of those blocks for the standard error and the one-sided p-value of r
    # (0: none, else >= 2), drawn from score_bootstrap_seed; score_save_predictions: the .npz also holds every prediction
    score_block: int = 128
    score_bootstrap: int = 0
    score_bootstrap_seed: int = 0
    score_save_predictions: bool = False

    def __post_init__(self):
        self.dtype = torch.bfloat16      # reference :155
        self.device_map = "auto"         # reference :157 (degenerate on one device)
        if self.cache_features and (self.use_lora or not self.freeze_backbone):
            raise ValueError("cache_features=True needs a frozen backbone without LoRA (freeze_backbone=True, use_lora=False): "
                             "with LoRA or a full fine-tune the backbone's output changes every step")
        if self.merge_lora_for_eval and not self.use_lora:
            raise ValueError("merge_lora_for_eval=True needs use_lora=True: without adapters there is nothing to merge")
        check_loss(self.loss, self.num_target)
        if self.ridge_fit is not None:
            if self.ridge_fit != "closed_form":
                raise ValueError(f"ridge_fit={self.ridge_fit!r}: expected None or 'closed_form'")
            if not self.cache_features:
                raise ValueError("ridge_fit='closed_form' reads the train split's frozen-feature cache: set cache_features=True "
                                 "(with freeze_backbone=True, use_lora=False)")
            if self.loss != "mse":
                raise ValueError(f"ridge_fit='closed_form' minimises the mse objective, loss={self.loss!r} has no closed form: "
                                 "set loss='mse' (or ridge_fit=None)")
            if not self.l2_lambda > 0:
                raise ValueError(f"ridge_fit='closed_form' needs l2_lambda > 0 (got {self.l2_lambda}): with fewer clips than "
                                 "features the system is singular without the penalty; set l2_lambda to a positive value")
        if isinstance(self.ridge_cv_folds, bool) or not isinstance(self.ridge_cv_folds, int) or self.ridge_cv_folds < 2:
            raise ValueError(f"ridge_cv_folds={self.ridge_cv_folds!r}: an integer >= 2 is needed")
        if isinstance(self.ridge_cv_block, bool) or not isinstance(self.ridge_cv_block, int) or self.ridge_cv_block < 1:
            raise ValueError(f"ridge_cv_block={self.ridge_cv_block!r}: an integer >= 1 is needed")
        if isinstance(self.score_block, bool) or not isinstance(self.score_block, int) or self.score_block < 1:
            raise ValueError(f"score_block={self.score_block!r}: an integer >= 1 is needed")
        if isinstance(self.score_bootstrap, bool) or not isinstance(self.score_bootstrap, int) or self.score_bootstrap < 0 \
                or self.score_bootstrap == 1:
            raise ValueError(f"score_bootstrap={self.score_bootstrap!r}: 0 (no bootstrap) or an integer >= 2 is needed")
        if isinstance(self.score_bootstrap_seed, bool) or not isinstance(self.score_bootstrap_seed, int) or self.score_bootstrap_seed < 0:
            raise ValueError(f"score_bootstrap_seed={self.score_bootstrap_seed!r}: an integer >= 0 is needed")
        if not isinstance(self.score_save_predictions, bool):
            raise ValueError(f"score_save_predictions={self.score_save_predictions!r}: true or false is needed")
        if self.ridge_lambda_grid is not None:
            if self.ridge_fit != "closed_form":
                raise ValueError("ridge_lambda_grid is the closed-form fit's choice of l2_lambda: set ridge_fit='closed_form' "
                                 "(or leave ridge_lambda_grid unset)")
            if isinstance(self.ridge_lambda_grid, (str, bytes)) or not hasattr(self.ridge_lambda_grid, "__iter__"):
                raise ValueError(f"ridge_lambda_grid={self.ridge_lambda_grid!r}: a list of l2_lambda values is needed")
            grid = list(self.ridge_lambda_grid)
            for x in grid:
                if isinstance(x, bool) or not isinstance(x, (int, float)) or not (math.isfinite(x) and x > 0):
                    raise ValueError(f"ridge_lambda_grid={grid!r}: {x!r} is not a positive number; every value must be > 0")
            grid = [float(x) for x in grid]
            if len(set(grid)) < 2 or len(set(grid)) != len(grid):
                raise ValueError(f"ridge_lambda_grid={grid!r}: two or more distinct values are needed")
            self.ridge_lambda_grid = grid
        if not isinstance(self.ridge_lambda_per_target, bool):
            raise ValueError(f"ridge_lambda_per_target={self.ridge_lambda_per_target!r}: true or false is needed")
        if self.ridge_lambda_per_target and self.ridge_lambda_grid is None:
            raise ValueError("ridge_lambda_per_target=True chooses each target's l2_lambda from ridge_lambda_grid: set "
                             "ridge_lambda_grid (or leave ridge_lambda_per_target unset)")
        if not isinstance(self.ridge_fit_weighted, bool):
            raise ValueError(f"ridge_fit_weighted={self.ridge_fit_weighted!r}: true or false is needed")
        if self.ridge_fit_weighted and self.ridge_fit != "closed_form":
            raise ValueError("ridge_fit_weighted=True is the closed-form fit under target weights: set ridge_fit='closed_form' "
                             "(or leave ridge_fit_weighted unset)")
        self.optimizer_groups = normalize_optimizer_groups(self.optimizer_groups)      # names are checked by configure_optimizers
        if self.ema_decay is not None:
            d = self.ema_decay
            if isinstance(d, bool) or not isinstance(d, (int, float)) or not 0 < d < 1:
                raise ValueError(f"ema_decay={d!r}: a number with 0 < ema_decay < 1 is needed (0.999 is usual; leave it unset for "
                                 "no moving average)")
            self.ema_decay = float(d)
            for name in ("ema_warmup", "ema_eval"):
                if not isinstance(getattr(self, name), bool):
                    raise ValueError(f"{name}={getattr(self, name)!r}: true or false is needed")
            if not self.freeze_backbone and not self.use_lora:
                raise ValueError(FULLFT_EMA_MESSAGE)
        if self.subjects is not None:
            self.subjects = list(check_subjects(self.subjects))
        if self.target_weights is not None:
            tw = self.target_weights
            if not isinstance(tw, str) or not tw.endswith(".npy"):
                raise ValueError(f"target_weights={tw!r}: the path of a .npy file is needed (leave it unset for no weights)")
            if "{subject}" in tw and self.subjects is None:
                raise ValueError(f"target_weights={tw!r} holds {{subject}} but `subjects` is unset: one subject takes one file "
                                 "of [num_target] weights")
            if self.ridge_fit is not None and not self.ridge_fit_weighted:
                raise ValueError("target_weights with ridge_fit='closed_form' needs ridge_fit_weighted=True: without it the "
                                 "closed-form fit and its cross-validation take every target alike (a mask needs NaN-tolerant "
                                 "Gram columns, general weights one factorisation per distinct weight); set "
                                 "ridge_fit_weighted=True or unset one of the two")
        if self.readout_layers is not None:
            if not self.freeze_backbone and not self.use_lora:
                raise ValueError("readout_layers with the full fine-tune (freeze_backbone=False, use_lora=False) is not supported: "
                                 "the connector and embedding backward below a tapped layer is out of scope.  Use "
                                 "freeze_backbone=True or use_lora=True")
            # the geometry name fixes L here already; configure_model checks again against the geometry it builds
            self.readout_layers = check_readout_layers(self.readout_layers, resolve_geometry(self).layers)


def load_target_weights(path: str, num_target: int, subjects=None) -> torch.Tensor:
    """``config.target_weights`` -> fp32 CPU tensor [num_target], or [G, num_target] with ``subjects``.  ``{subject}`` in the path
    (subjects only) names one [num_target] file per subject.  Shape, finiteness and sign are checked here with the file named;
    the head checks once more what a row must hold for its objective."""
    import numpy as np

    def one(p, shapes):
        if not os.path.isfile(p):
            raise ValueError(f"target_weights: {p!r} does not exist")
        a = np.load(p, allow_pickle=False)
        if a.dtype.kind not in "fiub" or tuple(a.shape) not in shapes:
            raise ValueError(f"target_weights: {p!r} holds {a.dtype} {tuple(a.shape)}, expected numbers of shape "
                             f"{' or '.join(str(list(s)) for s in shapes)}")
        a = a.astype(np.float32)
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError(f"target_weights: {p!r}: every weight must be finite and >= 0")
        return torch.from_numpy(a)
    V = int(num_target)
    if subjects is None:
        return one(path, ((V,),))
    if "{subject}" in path:
        return torch.stack([one(path.replace("{subject}", s), ((V,),)) for s in subjects])
    return one(path, ((V,), (len(subjects), V)))


def check_batch_subjects(batch, subjects, B: int | None = None):
    """The per-clip head index of a batch, checked on the host: -> None for a single-subject module, else an int64 CPU tensor
    [B] with values in [0, len(subjects)).  A batch with "subject" reaching a module without ``subjects``, or the reverse, is a
    configuration error (the module's and the datamodule's ``subjects`` must be the same list)."""
    has = "subject" in batch
    if has != (subjects is not None):
        raise ValueError(f"the batch {'carries' if has else 'has no'} \"subject\" but litmodule.config.subjects is "
                         f"{None if subjects is None else list(subjects)!r}: set litmodule.config.subjects and "
                         "datamodule.config.subjects to the same list (or leave both unset for one subject)")
    if subjects is None:
        return None
    idx = torch.as_tensor(batch["subject"]).detach().cpu().flatten()
    if idx.is_floating_point() or idx.dtype == torch.bool:
        raise ValueError(f"batch[\"subject\"] is {idx.dtype}: integer indices into subjects={list(subjects)!r} are needed")
    idx = idx.to(torch.int64)
    if B is not None and idx.numel() != B:
        raise ValueError(f"batch[\"subject\"] has {idx.numel()} entries for a batch of {B} clips")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(subjects)):
        raise ValueError(f"batch[\"subject\"]={idx.tolist()!r}: an index outside [0, {len(subjects)}) (subjects={list(subjects)!r})")
    return idx


def resolve_geometry(cfg: VLBLitModuleConfig) -> Geometry:
    kw = dict(num_target=cfg.num_target, l2_lambda=cfg.l2_lambda)
    if cfg.use_lora:
        kw.update(lora_r=cfg.lora_r, lora_alpha=cfg.lora_alpha)
    return geometry_mini(**kw) if cfg.geometry == "mini" else geometry_7b(**kw)


class _Attr:
    """Tiny namespace so ``self.nnmodule.config.hidden_size`` etc. read as in the reference."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


class VLBLitModule(_Base):
    def __init__(self, config: VLBLitModuleConfig) -> None:
        super().__init__()
        self.config = config
        from .parallel import local_device_index
        self._device = torch.device("cuda", local_device_index())
        self._step = 0
        self.world_size = 1
        self.rank = 0
        self.pack_tokens = bool(getattr(config, "pack_tokens", True))
        self._accumulate = None         # accumulate_grad_batches when set by hand; None: the attached runner's value
        self._micro = 0                 # position inside the current accumulation window
        self._window_opt_step = 0       # optimiser step count the position belongs to (a step() starts a new window)
        self.last_micro_batch = None    # runner's notice for the next training_step: it closes its window (True / False)

    @property
    def device(self):
        return self._device

    # ------------------------------------------------------------------ gradient accumulation
    @property
    def accumulate_grad_batches(self) -> int:
        """k: ``training_step`` calls per optimiser step.  Not a config field (the 16 are the reference's): it is the
        ``accumulate_grad_batches`` of the runner that drives the module (``lightning.pytorch.Trainer`` or the built-in
        ``trainer.Trainer``), or a value set here by a hand-written loop."""
        if self._accumulate is not None:
            return self._accumulate
        tr = self.__dict__.get("_trainer") or self.__dict__.get("trainer")
        k = getattr(tr, "accumulate_grad_batches", 1)
        return 1 if k is None else check_accumulate_grad_batches(k)

    @accumulate_grad_batches.setter
    def accumulate_grad_batches(self, k):
        self._accumulate = None if k is None else check_accumulate_grad_batches(k)

    def check_accumulation_supported(self, k: int | None = None):
        """k > 1 is refused where there is nowhere to accumulate: the full fine-tune under data parallelism."""
        k = self.accumulate_grad_batches if k is None else k
        sb = getattr(self, "sharded_backbone", None)
        if k > 1 and sb is not None and sb.active:
            raise ValueError(f"accumulate_grad_batches={k} with the full fine-tune under data parallelism is not supported "
                             f"({'FULL_SHARD' if sb.full_shard else 'SHARD_GRAD_OP'}: the layers' bf16 gradient "
                             f"{'buffers rotate' if sb.full_shard else 'shards are reduce-scattered'} every step and have nowhere to "
                             "accumulate).  Use accumulate_grad_batches=1 and more ranks for the batch size, or train LoRA / the "
                             "frozen-backbone head, which accumulate under data parallelism")

    # ------------------------------------------------------------------ model
    def configure_model(self, state_dict: dict | None = None, head_state: dict | None = None) -> None:
        """reference :206-226.  The hub checkpoint is unreachable offline: weights are
        random-initialised on the device unless a state dict (upstream naming) is handed in.  Head tensors
        (``layer_norm1.weight`` ...) and adapters (peft layout: ``...lora_A.weight`` [r,in], ``...lora_B.weight``
        [out,r]) are taken from ``head_state`` or, when present there, from ``state_dict`` itself - so a
        ``trainable_state_dict()`` / checkpoint ``state_dict`` merged into the backbone's loads back unchanged."""
        if getattr(self, "nnmodule", None) is not None:
            return
        cfg = self.config
        # reference :86-111: freeze_backbone=False and use_lora=False -> everything but the vision tower trains
        full_ft = not cfg.freeze_backbone and not cfg.use_lora
        g = self.geometry = resolve_geometry(cfg)
        dev = self.device
        torch.cuda.set_device(dev)
        if state_dict is None:
            if cfg.model_path and os.path.isdir(cfg.model_path):
                state_dict = load_safetensors_dir(cfg.model_path)
            else:
                warnings.warn(f"model_path={cfg.model_path!r} is not a local directory: random-initialising "
                              f"the {cfg.geometry} architecture (no network / HF cache in this environment)")
                state_dict = Weights.random_state_dict(g, dev, seed=cfg.init_seed)
        weights = Weights(g, state_dict, dev, keep_transposed=bool(cfg.use_lora) or full_ft, gate_up_interleaved=not full_ft)
        lora_state = {k: v for k, v in state_dict.items() if ".lora_" in k} or None
        taps = check_readout_layers(getattr(cfg, "readout_layers", None), g.layers)
        if taps is not None and full_ft:
            raise ValueError("readout_layers with the full fine-tune (freeze_backbone=False, use_lora=False) is not supported")
        if head_state is None and all(n in state_dict for n in HEAD_PARAMS):
            # layer_mix.weight is optional on load: a checkpoint from before the taps starts from the uniform mix
            head_state = {n: state_dict[n] for n in HEAD_PARAMS + (LAYER_MIX,) if n in state_dict}
        del state_dict
        self.backbone = Backbone(g, weights)
        self.nnmodule = _Attr(config=_Attr(hidden_size=g.dim, tokenizer_model_max_length=g.max_len,
                                           num_frames=g.num_frames, use_cache=False), backbone=self.backbone)
        self.head = BrainHead(g.dim, cfg.num_target, cfg.l2_lambda, g.ln_eps, dev, sd=head_state, seed=cfg.init_seed,
                              loss=getattr(cfg, "loss", "mse"), readout_layers=taps, subjects=getattr(cfg, "subjects", None))
        if "_ridge_cv_lambda" in self.__dict__:      # a checkpoint loaded before the head existed: the l2_lambda its fit chose
            self.head.l2_lambda = float(self.__dict__["_ridge_cv_lambda"])
        if "_ridge_lambda_rows" in self.__dict__:    # likewise the per-target penalties (ridge_lambda_per_target, §5.3.7)
            self.head.set_l2_lambda_rows(self.__dict__["_ridge_lambda_rows"].to(dev, torch.float32))
        # per-target loss weights (§5.3.8): the configured file, and / or what a checkpoint loaded before the head existed held
        tw = self.__dict__.get("_target_weights")
        if getattr(cfg, "target_weights", None) is not None:
            filed = load_target_weights(cfg.target_weights, cfg.num_target, getattr(cfg, "subjects", None))
            self._check_same_weights(filed, tw, cfg.target_weights)
            tw = filed
        if tw is not None:
            self.set_target_weights(tw)
        # reference attribute names
        self.hrf_layer = self.head
        self.ridge_layer = self.head
        self.layer_norm1 = self.head
        self.layer_norm2 = self.head
        self.dropout = _Attr(p=cfg.dropout_rate)
        self.lora = self.full = None
        if full_ft:
            from .fullft import FullFineTune
            self.full = FullFineTune(g, self.backbone, dev, fp8_gemm=bool(getattr(cfg, "fp8_gemm", False)))
        if cfg.use_lora:
            from .lora import LoraState
            lora_sd = None if head_state is None and lora_state is None else {**(head_state or {}), **(lora_state or {})}
            self.lora = LoraState(g, weights, cfg.lora_r, cfg.lora_alpha, cfg.lora_dropout or 0.0, dev, seed=cfg.init_seed,
                                  sd=lora_sd, target_modules=find_all_linear_names(self.backbone))

    # ------------------------------------------------------------------ per-target loss weights and masks
    def set_target_weights(self, tw) -> None:
        """``tw``: [num_target], or [G, num_target] with ``subjects`` (a tensor on any device, or anything torch.as_tensor takes);
        None: no weights.  Goes to ``BrainHead.set_target_weights`` (which checks it) and into checkpoints.  With
        ``ridge_fit_weighted`` the closed-form fit takes the weights in force when it runs and a head may hold at
        most 8 distinct positive ones; weights set after a completed fit do not refit: the parameters stay the minimiser of the
        objective they were fitted to and only the steps and scores from then on use the new weights."""
        weighted_fit = bool(getattr(self.config, "ridge_fit_weighted", False))
        if tw is not None and getattr(self.config, "ridge_fit", None) is not None and not weighted_fit:
            raise ValueError("set_target_weights with ridge_fit='closed_form' needs ridge_fit_weighted=True: without it the "
                             "closed-form fit takes every target alike")
        t = None if tw is None else torch.as_tensor(tw).detach().to("cpu", torch.float32).clone()
        if t is not None and weighted_fit and t.dim() in (1, 2) and bool((torch.isfinite(t) & (t >= 0)).all()):
            subs = getattr(self.config, "subjects", None)       # more than 8 levels: refused here, before epoch 1
            target_weight_levels(t.reshape(-1, t.shape[-1]),
                                 (lambda g: f"head {g} ({subs[g]!r})") if subs is not None and t.dim() == 2 and t.shape[0] > 1
                                 else (lambda g: "the head"))
        head = getattr(self, "head", None)
        if head is not None:
            head.set_target_weights(None if t is None else t.to(head.dev))
            t = None if t is None else head.tw.detach().cpu().clone()       # [max(1,G), num_target], as the head keeps it
        if t is None:
            self.__dict__.pop("_target_weights", None)
        else:
            self._target_weights = t

    def target_weight_mask(self):
        """host bool [max(1,G), num_target]: True where a target's weight is positive; None without weights"""
        t = self.__dict__.get("_target_weights")
        return None if t is None else (t.reshape(-1, t.shape[-1]) > 0)

    def _check_same_weights(self, filed, other, path) -> None:
        """a checkpoint's weights against the configured file's: they must be the same numbers"""
        if filed is None or other is None:
            return
        V = filed.shape[-1]
        a, b = filed.reshape(-1, V), other.reshape(-1, other.shape[-1])
        n = max(a.shape[0], b.shape[0])
        if b.shape[-1] != V or a.shape[0] not in (1, n) or b.shape[0] not in (1, n) or not torch.equal(a.expand(n, V), b.expand(n, V)):
            raise ValueError(f"the checkpoint's vlb_target_weights differ from target_weights={path!r}: resume with the file "
                             "the run was trained with, or unset target_weights to take the checkpoint's")

    def _named_masters(self):
        """(name, fp32 master tensor) of everything AdamW updates: head always; LoRA A/B when use_lora
        (reference :86-120: backbone frozen / peft freezes the base)."""
        out = [(n, self.head.master[n]) for n in self.head.param_names]
        if self.lora is not None:
            out += self.lora.named_masters()
        if self.full is not None:       # full fine-tune: every backbone tensor outside the vision tower (kernel layouts)
            f = self.full.flat
            if f.master is None:        # FULL_SHARD (parallel.attach_data_parallel): no full-size master; the handles are placeholders
                cache = self.__dict__.get("_param_cache", {})
                out += [(f"backbone.{n}", cache[f"backbone.{n}"].data) for n in f.offsets if f"backbone.{n}" in cache]
            else:
                out += [(f"backbone.{n}", f.view(f.master, n)) for n in f.offsets]
        return out

    def trainable_named_parameters(self):
        """(name, ``nn.Parameter``) of the trainables.  Each Parameter ALIASES its fp32 master (the flat buffer the fused
        AdamW updates in place): the objects are stable across calls, so an optimiser's ``param_groups``, Lightning's
        ``zero_grad`` / ``loss.backward()`` and ``.grad`` all refer to the same things; they are re-made only when a master
        moved (``configure_optimizers`` re-points the masters into the flat store)."""
        cache = self.__dict__.setdefault("_param_cache", {})
        out = []
        for n, t in self._named_masters():
            hit = cache.get(n)
            if hit is None or hit.data_ptr() != t.data_ptr() or hit.shape != t.shape:
                hit = cache[n] = torch.nn.Parameter(t, requires_grad=True)
            out.append((n, hit))
        return out

    def parameters(self, recurse: bool = True):
        return [p for _, p in self.trainable_named_parameters()]

    def _attach_gradients(self):
        """``.grad`` of every trainable Parameter <- the gradient buffer the explicit backward filled (aliases, no copies)."""
        masters = dict(self._named_masters())
        opt = getattr(self, "optimizer", None)
        acc = opt.window_gradient(0) if opt is not None and self._window_complete() else None
        for n, p in self.trainable_named_parameters():
            if n.startswith("backbone."):
                continue        # bf16 gradients (like the reference's bf16 parameters'): read them with self.full.flat.g_(name)
            if acc is not None:             # a complete accumulation window: what the optimiser will consume is the accumulator
                o, cnt, shp = self.flat.offsets[n]
                g = acc[o:o + cnt].view(shp)
            else:
                g = self.head.grads[n] if n in self.head.grads else self.lora.grads[n]
            p.grad = g
            masters[n].grad = g             # the plain master views (head.master[n], lora.master[n]) carry it too

    def _window_complete(self) -> bool:
        k = self.accumulate_grad_batches
        return k > 1 and (self._micro >= k or bool(self.__dict__.get("_window_closed")))

    def trainable_state_dict(self, averaged: bool = False) -> dict:
        """Trainables on the host under their upstream / peft names and layouts (LoRA B as [out, r], rank padding
        removed): what checkpoints store and what ``configure_model(state_dict=...)`` / peft accept.  ``averaged``: the
        moving average of every tensor (``ema_decay``) in place of its master, same names and layouts."""
        if averaged:
            ema = self._ema_buffer()
            if ema is None:
                raise ValueError("trainable_state_dict(averaged=True) needs litmodule.config.ema_decay and configure_optimizers(): "
                                 "there is no moving average")
            view = lambda n: self.flat.view(ema, n)            # noqa: E731
            sd = {n: view(n).detach().cpu().clone() for n in self.head.param_names}
            if self.lora is not None:
                sd.update({n: t.cpu() for n, t in self.lora.state_dict({n: view(n) for n in self.lora.master}).items()})
            return sd
        sd = {n: self.head.master[n].detach().cpu().clone() for n in self.head.param_names}
        if self.lora is not None:
            sd.update({n: t.cpu() for n, t in self.lora.state_dict().items()})
        if self.full is not None:
            sd.update(self.full.state_dict())
        return sd

    def load_trainable_state_dict(self, sd: dict) -> None:
        """Inverse of ``trainable_state_dict`` into the fp32 masters; bf16 copies and derived layouts are rebuilt."""
        for n in self.head.param_names:
            self.head.master[n].copy_(sd[n].to(self.device, torch.float32))
            self.head.compute[n].copy_(self.head.master[n])
        if self.lora is not None:
            self.lora.load_state_dict(sd)
        # full fine-tune: the backbone masters travel as the flat store itself (trainer.trainable_state 'stores')

    # ------------------------------------------------------------------ weight averaging (ema_decay)
    def _ema_buffer(self):
        """The optimiser's flat fp32 moving average of the trainables, or None (no ``ema_decay``, no optimiser yet)."""
        return getattr(getattr(self, "optimizer", None), "ema", None)

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the context every forward reads the moving average of the trainables instead of the last iterate: the
        bf16 compute buffer of the flat store is stashed, ``bf16(ema)`` is written over it and the optimiser's ``post_step``
        callables rebuild what is derived from it (LoRA's A^T / B layouts; ``lora.version`` moves, so ``merge()`` re-merges).
        On exit, after an exception too, the stash is copied back and ``post_step`` runs again: the restored copies are the
        stashed bits, not a re-cast of the masters.  Masters, moments and the average itself are never touched.  Without
        ``ema_decay``, and when entered a second time inside itself, it does nothing."""
        ema = self._ema_buffer()
        if ema is None or self.__dict__.get("_ema_swapped", False):
            yield
            return
        from ._lib import check, lib
        compute, opt = self.flat.compute, self.optimizer
        stash = self.__dict__.get("_ema_stash")
        if stash is None or stash.numel() != compute.numel():
            stash = self._ema_stash = torch.empty_like(compute)
        stash.copy_(compute)
        self._ema_swapped = True
        try:
            check(lib.vlb_cast_f32_to_bf16(ema.data_ptr(), compute.data_ptr(), ema.numel(), ops._stream()), "vlb_cast_f32_to_bf16")
            for fn in opt.post_step:
                fn()
            yield
        finally:
            compute.copy_(stash)
            for fn in opt.post_step:
                fn()
            self._ema_swapped = False

    def _eval_weights(self):
        """``averaged_weights()`` when ``ema_eval`` asks validation and the merged export to read the average, else nothing."""
        return self.averaged_weights() if getattr(self.config, "ema_eval", False) else contextlib.nullcontext()

    def log_ema_decay(self):
        """``ema/decay``, the decay of the last EMA update, once per validation epoch (both runners call this at its end)."""
        d = getattr(getattr(self, "optimizer", None), "ema_last_decay", None)
        if d is not None:
            self.log("ema/decay", float(d))

    # ------------------------------------------------------------------ dropout randomness (counter based)
    def _dropout_seed(self) -> int:
        """Head dropout seed of the current step: (init_seed, rank, step) - ranks draw different masks for their
        clips and a resumed run continues the sequence from the restored step counter."""
        x = (self.config.init_seed * 0x9E3779B1 + (self.rank + 1) * 0x7F4A7C15 + self._step * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF
        return x or 1

    def rng_state(self) -> dict:
        return {"head_step": self._step, "lora_step": None if self.lora is None else self.lora.step}

    def set_rng_state(self, st: dict) -> None:
        self._step = int(st.get("head_step", 0))
        if self.lora is not None and st.get("lora_step") is not None:
            self.lora.step = int(st["lora_step"])

    # ------------------------------------------------------------------ pieces of the step
    def make_weight_mask(self, pad_vals, vis_weights, lang_weights, lang_len, max_len):
        """reference :178-203 - one launch; values rounded to bf16 like the reference's mask."""
        g = self.geometry
        feature_len = vis_weights.shape[1] * g.ds_grid * g.ds_grid + lang_len - 1
        assert feature_len == max_len
        dev = self.device
        return ops.weight_mask(pad_vals.to(dev, torch.int64), vis_weights.to(dev, torch.float64),
                               lang_weights.to(dev, torch.float64), g.ds_grid * g.ds_grid, max_len, round_bf16=True)

    def _vision_tensor(self, x_video):
        if isinstance(x_video, (list, tuple)):          # reference passes [(tensor, "video"), ...]
            x_video = torch.stack([v[0] if isinstance(v, (list, tuple)) else v for v in x_video])
        return x_video.to(self.device, torch.float32).contiguous()

    def forward(self, x_video, x_lang, weight_mask, attention_mask=None, y=None, keep_scale=None, layout=None, ids_host=None,
                subject=None):
        """reference :229-256 -> (regression_output fp32 [B,V], l2_reg).  attention_mask is re-derived
        on the device from the ids (ids != 0), exactly what the reference passes in (:271).
        ``layout``: packed RowLayout from ``backbone.row_layout`` (rows without padded tails).  ``subject``: with
        ``config.subjects``, the head index of every clip (host ints or a CPU tensor [B]); checked before anything is launched."""
        if (subject is None) != (self.head.G == 0):
            self.head._group(subject, x_lang.shape[0])          # raises: a multi-subject head needs `subject`, a single one takes none
        vis = self._vision_tensor(x_video)
        ids = x_lang.to(self.device, torch.int64).contiguous()
        B = ids.shape[0]
        taps = self.head.readout_layers
        tap_kw = {}
        if taps is not None:
            # the decoder stops at the highest tap; every tapped layer is pooled as soon as it exists (nothing is kept here)
            self.head.begin(*weight_mask.shape)
            tap_kw = dict(stop=taps[-1], on_layer=lambda k, h: self.head.tap(taps.index(k), h, weight_mask, layout) if k in taps else None)
        if self.lora is not None and not self.training and getattr(self.config, "merge_lora_for_eval", False):
            hidden, key_mask = self._merged_forward(vis, ids, layout, **tap_kw)      # the same adapters, folded into the weights
        elif self.lora is not None:      # eval mode keeps the adapters (peft eval: dropout off), like the reference's validation
            hidden, key_mask = self.lora.forward(self.backbone, vis, ids, layout, train=self.training, **tap_kw)
        elif self.full is not None and self.training:      # full fine-tune: forward that keeps what backward needs
            hidden, key_mask = self.full.forward(vis, ids, layout, ids_host=ids_host)
        else:
            hidden, key_mask = self.backbone.forward(vis, ids, layout=layout, **tap_kw)
        if y is None:
            y = torch.zeros(B, self.config.num_target, dtype=torch.float32, device=self.device)
        if taps is not None:
            pred, terms = self.head.forward_tapped(y, keep_scale, subject)
        else:
            pred, terms = self.head.forward(hidden, weight_mask, y, keep_scale, layout, subject)
        self._loss_terms = terms
        return pred, terms[1]

    # ------------------------------------------------------------------ merged adapters (peft merge_adapter / merge_and_unload)
    def _merged_layers(self):
        """``LoraState.merge()``'s per-layer weights (re-merged only when the adapters changed since the last merge)."""
        if self.lora is None:
            raise ValueError("merged weights need a LoRA run (use_lora=True): there are no adapters to merge")
        if getattr(self.backbone, "store", None) is not None:
            raise ValueError("merged LoRA weights with a sharded frozen layer store (Backbone.enable_sharding) are not supported: "
                             "every rank holds 1/world of each layer, and merging gathered shards is out of scope")
        return self.lora.merge()

    def _merged_forward(self, vis, ids, layout, stop=None, on_layer=None):
        """Eval-mode forward of a LoRA module on merged weights: the frozen path (``Backbone.decoder_layer``: one GEMM per
        projection, SwiGLU in the epilogue) instead of ``LoraState.decoder_forward(train=False)``."""
        bb, g = self.backbone, self.geometry
        layers = self._merged_layers()
        emb, key_mask = bb.splice(ids, bb.video_tokens(vis), layout)
        tap_kw = {} if stop is None and on_layer is None else dict(stop=stop, on_layer=on_layer)
        return bb.decoder(emb, key_mask, vis.shape[0], g.max_len, layout=layout, layers=layers, **tap_kw), key_mask

    def merged_state_dict(self) -> dict:
        """The decoder linears with the adapters merged in (``W + (alpha/r) B A``, bf16, host) under their upstream names,
        de-stacked and de-interleaved, plus the head tensors: with the untouched rest of the base checkpoint it loads as a
        plain decoder, ``configure_model(state_dict={**base, **merged})`` under ``use_lora=False, freeze_backbone=True``.
        With ``ema_decay`` and ``ema_eval`` the adapters and the head tensors are their moving averages."""
        sd = {}
        averaged = self._ema_buffer() is not None and bool(getattr(self.config, "ema_eval", False))
        with self._eval_weights():          # ema_decay + ema_eval: the averaged adapters (and head), as validation reads them
            for i, mw in enumerate(self._merged_layers()):
                lins = destack_decoder_layer(self.geometry, mw["wqkv"], mw["wo"], mw["wdown"], mw.get("wgu"), mw.get("wgu_il"))
                for n, t in lins.items():
                    sd[f"model.layers.{i}.{n}.weight"] = t.detach().cpu().contiguous().clone()
        if averaged:
            sd.update({n: self.flat.view(self._ema_buffer(), n).detach().cpu().clone() for n in self.head.param_names})
        else:
            sd.update({n: self.head.master[n].detach().cpu().clone() for n in self.head.param_names})
        return sd

    def save_merged(self, path: str) -> str:
        """``merged_state_dict()`` as one safetensors file (the format ``load_safetensors_dir`` reads)."""
        from safetensors.torch import save_file
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        save_file(self.merged_state_dict(), path)
        return path

    def _common_step(self, batch, train: bool, use_cache: bool = True):
        """``use_cache=False`` (the evaluation pass): the feature cache is not consulted, the clip runs the backbone"""
        cfg, g = self.config, self.geometry
        dev = self.device
        self._cached_step = False
        subject = check_batch_subjects(batch, getattr(cfg, "subjects", None), len(batch["timeseries"]))
        cache = self.feature_caches.get("train" if train else "val") if cfg.cache_features and use_cache and "index" in batch else None
        if cache is not None and cache.lookup(batch["index"]):
            # every clip's features are cached: no backbone, no weight mask; the same head kernels on the same fp32 inputs
            y = batch["timeseries"].to(dev, torch.float32).to(torch.bfloat16).float().contiguous()
            keep = None
            if train and cfg.dropout_rate > 0:
                keep = ops.dropout_keep_scale(y.shape[0], g.dim, cfg.dropout_rate, self._dropout_seed(), dev)
            if torch.is_tensor(batch.get("vision")):
                self.discard_prefetched_vision(batch)       # its frozen vision side is not needed
            pred, terms = self.head.forward_cached(cache, batch["index"], y, keep, subject)
            self._loss_terms = terms
            self._cached_step = True
            return pred, y, terms
        if cache is not None and "vision" not in batch:
            raise RuntimeError(f"feature cache {cache.split!r}: a features-only batch missed the cache (indices "
                               f"{batch['index'].tolist()})")
        # unpadded (packed) rows, like the reference's flash-attn path; needs the ids on the host (no sync)
        layout = self.backbone.row_layout(batch["language"], batch["padvals"]) if self.pack_tokens else None
        x_lang = batch["language"].to(dev).long()
        wm = self.make_weight_mask(batch["padvals"], batch["vis_weights"], batch["lang_weights"], x_lang.shape[1],
                                   self.nnmodule.config.tokenizer_model_max_length)
        y = batch["timeseries"].to(dev, torch.float32).to(torch.bfloat16).float().contiguous()   # reference :288
        keep = None
        if train and cfg.dropout_rate > 0:          # nn.Dropout(p) in training mode (reference :226,251)
            keep = ops.dropout_keep_scale(x_lang.shape[0], g.dim, cfg.dropout_rate, self._dropout_seed(), dev)
        ids_host = batch["language"] if batch["language"].device.type == "cpu" else None
        pred, _ = self.forward(batch["vision"], x_lang, wm, y=y, keep_scale=keep, layout=layout, ids_host=ids_host, subject=subject)
        if cache is not None and cache.store(batch["index"], self.head) and cache.complete() and cfg.feature_cache_dir:
            cache.save(cfg.feature_cache_dir, self._feature_cache_fp[cache.split])
        return pred, y, self._loss_terms

    # ------------------------------------------------------------------ frozen-backbone feature cache (feature_cache.py)
    @property
    def feature_caches(self) -> dict:
        return self.__dict__.setdefault("_feature_caches", {})

    def setup_feature_cache(self, train_dataset=None, val_dataset=None) -> None:
        """One FeatureCache per split, sized by its dataset; with ``feature_cache_dir`` each is filled from disk when the
        fingerprint there matches.  The datasets start handing out ``"index"``.  Called once per fit, after configure_model."""
        from .feature_cache import FeatureCache, fingerprint
        cfg = self.config
        if not cfg.cache_features:
            return
        fps = self.__dict__.setdefault("_feature_cache_fp", {})
        for split, ds in (("train", train_dataset), ("val", val_dataset)):
            if ds is None:
                continue
            ds.with_index = True
            c = self.feature_caches.get(split)
            if c is None or c.n != len(ds):
                c = self.feature_caches[split] = FeatureCache(split, len(ds), self.geometry.dim, self.device,
                                                              layers=self.head.K or None)     # one slab per tapped layer
            fps[split] = fingerprint(cfg, ds)
            if cfg.feature_cache_dir and not c.complete():
                c.load(cfg.feature_cache_dir, fps[split])
        if cfg.ridge_fit is not None and train_dataset is not None:
            self._ridge_fit_dataset, self._ridge_fit_done = train_dataset, False
            self._maybe_fit_ridge()            # a persisted cache is complete already: the fit precedes the first step

    def _maybe_fit_ridge(self) -> None:
        """ridge_fit="closed_form": run the fit once per fit, the first time the train split's cache is complete."""
        if self.config.ridge_fit is None or self.__dict__.get("_ridge_fit_done", True):
            return
        c = self.feature_caches.get("train")
        if c is None or not c.complete():
            return
        self._ridge_fit_done = True
        self.fit_ridge_closed_form(self._ridge_fit_dataset)

    def fit_ridge_closed_form(self, dataset=None, l2_lambda=None, chunk: int = 512) -> list:
        """Set ``ridge_layer.linear.{weight,bias}`` to the minimiser of the mse objective over the train split, for the LN
        parameters (and the layer mix) as they are now and without dropout: walk ``dataset`` (default: the
        train dataset) in ``features_only`` mode in index order, ``chunk`` clips at a time, accumulate the fp64 sums from the
        cached features, solve per head, write the fp32 masters (wherever they live) and their bf16 copies, and zero AdamW's
        moments of exactly these two tensors.  Logs ``ridge_fit/n``, ``ridge_fit/l2_lambda`` and the first chunk's
        ``ridge_fit/train_mse_before`` / ``_after`` (the existing cached forward).  -> ``BrainHead.ridge_solve``'s list.
        With ``ridge_lambda_grid`` set and no explicit ``l2_lambda`` the same walk keeps the sums per fold, ``ridge_cv``
        chooses ``l2_lambda``, the solve uses it and ``head.l2_lambda`` keeps it; ``ridge_fit/cv_score``,
        ``/cv_score_<i>`` and ``/cv_best_index`` are logged too and ``ridge_fit_result`` is ``ridge_cv``'s dict.
        With ``ridge_lambda_per_target`` as well, ``ridge_cv(grid, per_target=True)`` chooses per (head, target),
        ``ridge_solve_rows`` solves each row with its own l2_lambda and ``head.set_l2_lambda_rows`` puts the vector in force
        (DESIGN §5.3.7); ``ridge_fit/cv_score_per_target`` and ``/lambda_count_<i>`` are logged too.  An explicit
        ``l2_lambda`` skips the grid and clears the vector.
        With ``ridge_fit_weighted`` and target weights set the same walk and the same calls minimise the
        weighted objective (NaN in a masked target is ignored); ``train_mse_before`` / ``_after`` are then its weighted data
        term and ``ridge_fit/kept_targets`` and ``/weight_levels`` (summed over heads) are logged too."""
        cfg = self.config
        if not cfg.cache_features or cfg.loss != "mse":
            raise ValueError("fit_ridge_closed_form needs cache_features=True and loss='mse'")
        cache = self.feature_caches.get("train")
        if cache is None or not cache.complete():
            raise RuntimeError("fit_ridge_closed_form: the train split's feature cache is not complete yet (it fills during "
                               "the first epoch, or loads from feature_cache_dir)")
        ds = dataset if dataset is not None else self.__dict__.get("_ridge_fit_dataset") or self._datamodule_dataset("train")
        if ds is None or len(ds) != cache.n:
            raise ValueError(f"fit_ridge_closed_form: a dataset of {None if ds is None else len(ds)} clips for a cache of {cache.n}")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"fit_ridge_closed_form: chunk={chunk}")
        subjects = getattr(cfg, "subjects", None)
        was = ds.features_only
        ds.features_only = True            # an item is {"index", "timeseries"[, "subject"]}: nothing else is read
        first = mse = cv = None
        # ridge_lambda_grid (and no explicit l2_lambda): the same one walk keeps the sums per fold, ridge_cv chooses (§5.3.6)
        grid = cfg.ridge_lambda_grid if l2_lambda is None else None
        try:
            weighted = bool(getattr(cfg, "ridge_fit_weighted", False))
            if grid is not None:
                self.head.ridge_stats_begin(folds=cfg.ridge_cv_folds, block=cfg.ridge_cv_block, weighted=weighted)
            else:
                self.head.ridge_stats_begin(weighted=weighted)
            wst = self.head._ridge if "tw" in self.head._ridge else None         # the weights this fit takes (§5.3.9)
            kept_levels = None if wst is None else (float(sum(wst["kept"])), float(sum(len(s) for s in wst["scale"])))
            for lo in range(0, len(ds), chunk):
                items = [ds[i] for i in range(lo, min(lo + chunk, len(ds)))]
                batch = {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in items[0]}
                subject = check_batch_subjects(batch, subjects, len(items))
                # the targets as every step sees them (reference :288: through bf16)
                y = batch["timeseries"].to(self.device, torch.float32).to(torch.bfloat16).float().contiguous()
                if first is None:
                    first = (batch["index"], y, subject)
                    mse = [float(self.head.forward_cached(cache, *first[:2], None, subject)[1][0])]
                self.head.ridge_stats_add(cache, batch["index"], y, subject)
            if grid is not None and cfg.ridge_lambda_per_target:
                cv = self.head.ridge_cv(grid, per_target=True)
                out = self.head.ridge_solve_rows(cv["choice"], grid)
                self.head.set_l2_lambda_rows(cv["lambda_rows"].flatten())
                self._ridge_lambda_rows = self.head.l2_lambda_rows.detach().cpu()
                self.head.l2_lambda = self._ridge_cv_lambda = float(cv["best_lambda"])       # the global choice, for reporting
            elif grid is not None:
                cv = self.head.ridge_cv(grid)
                out = self.head.ridge_solve(cv["best_lambda"])
                # every later step and validation loss uses the objective these weights minimise
                self.head.l2_lambda = self._ridge_cv_lambda = float(cv["best_lambda"])
            else:
                out = self.head.ridge_solve(cfg.l2_lambda if l2_lambda is None else l2_lambda)
            if not (grid is not None and cfg.ridge_lambda_per_target) and self.head.l2_lambda_rows is not None:
                self.head.set_l2_lambda_rows(None)               # a fit with one l2_lambda: one scalar penalty again
                self.__dict__.pop("_ridge_lambda_rows", None)
        finally:
            ds.features_only = was
            self.head.ridge_stats_end()
        opt = getattr(self, "optimizer", None)
        if opt is not None:
            opt.reset_moments(["ridge_layer.linear.weight", "ridge_layer.linear.bias"])
            opt.reset_ema(["ridge_layer.linear.weight", "ridge_layer.linear.bias"])      # ema_decay: the average restarts at the new values
        mse.append(float(self.head.forward_cached(cache, first[0], first[1], None, first[2])[1][0]))
        self.log("ridge_fit/n", float(sum(o["n"] for o in out)))
        self.log("ridge_fit/l2_lambda", float(out[0]["l2_lambda"]) if "l2_lambda" in out[0] else float(cv["best_lambda"]))
        self.log("ridge_fit/train_mse_before", mse[0])
        self.log("ridge_fit/train_mse_after", mse[1])
        if kept_levels is not None:
            self.log("ridge_fit/kept_targets", kept_levels[0])
            self.log("ridge_fit/weight_levels", kept_levels[1])
        if cv is not None:
            self.log("ridge_fit/cv_score", float(cv["score"][cv["best_index"]]))
            for i, s in enumerate(cv["score"]):
                self.log(f"ridge_fit/cv_score_{i}", float(s))
            self.log("ridge_fit/cv_best_index", float(cv["best_index"]))
            if "lambda_counts" in cv:
                self.log("ridge_fit/cv_score_per_target", float(cv["score_per_target"]))
                for i in range(len(cv["grid"])):
                    self.log(f"ridge_fit/lambda_count_{i}", float(sum(row[i] for row in cv["lambda_counts"])))
            self.ridge_fit_result = dict(cv, solve=out)     # ridge_cv's dict, and ridge_solve's list under "solve"
            return out
        self.ridge_fit_result = out
        return out

    def feature_cache_begin(self, split: str, dataset=None) -> None:
        """Start of a training epoch / validation pass: a split whose cache is complete stops loading anything but the
        targets (``features_only``; the loader's iterator - and its workers - are re-created per epoch and per pass)."""
        c = self.feature_caches.get(split)
        if c is None:
            return
        c.reset_counters()
        if dataset is not None:
            dataset.features_only = c.complete()

    def feature_cache_end(self, split: str) -> float | None:
        """End of a training epoch / validation pass: ``feature_cache/<split>_hit_rate`` (fraction of batches run from the
        cache) through ``log``."""
        c = self.feature_caches.get(split)
        rate = None if c is None else c.hit_rate()
        if rate is not None:
            self.log(f"feature_cache/{split}_hit_rate", rate)
        if split == "train" and self.config.ridge_fit is not None:
            self._maybe_fit_ridge()            # the epoch that completed the train cache ends with the closed-form fit
        return rate

    def _datamodule_dataset(self, split):
        dm = getattr(getattr(self, "trainer", None), "datamodule", None)
        return getattr(getattr(dm, "datasets", None), split, None)

    def on_train_epoch_start(self):
        """Lightning hook (the built-in runner calls feature_cache_begin itself)."""
        if self.config.cache_features:
            if not self.feature_caches:
                self.setup_feature_cache(self._datamodule_dataset("train"), self._datamodule_dataset("val"))
            self.feature_cache_begin("train", self._datamodule_dataset("train"))

    def on_train_epoch_end(self):
        if self.config.cache_features:
            self.feature_cache_end("train")

    def on_validation_epoch_start(self):
        """Lightning hook.  ``ema_decay`` with ``ema_eval``: the whole validation epoch runs inside ``averaged_weights()``."""
        if self.__dict__.get("_ema_val_ctx") is None and self._ema_buffer() is not None and getattr(self.config, "ema_eval", False):
            self._ema_val_ctx = self.averaged_weights()
            self._ema_val_ctx.__enter__()
        if self.config.cache_features:
            if not self.feature_caches:
                self.setup_feature_cache(self._datamodule_dataset("train"), self._datamodule_dataset("val"))
            self.feature_cache_begin("val", self._datamodule_dataset("val"))

    def on_validation_epoch_end(self):
        if self.config.cache_features:
            self.feature_cache_end("val")
        ctx, self._ema_val_ctx = self.__dict__.get("_ema_val_ctx"), None
        if ctx is not None:
            ctx.__exit__(None, None, None)         # back on the last iterate before any checkpoint callback runs
        self.log_readout_alpha()
        self.log_ema_decay()

    def log_readout_alpha(self):
        """``readout/alpha_<layer>`` = softmax(layer_mix.weight) of the bf16 copy the kernels read, once per validation
        epoch (both runners call this at its end); nothing without ``readout_layers``."""
        head = getattr(self, "head", None)
        taps = None if head is None else head.readout_layers
        if taps is None:
            return
        alpha = torch.softmax(head.compute[LAYER_MIX].float(), 0).tolist() if head.K > 1 else [1.0]
        for k, a in zip(taps, alpha):
            self.log(f"readout/alpha_{k}", a)

    def prefetch_vision(self, batch, ready_event=None):
        """Start the frozen vision side (CLIP tower + STC connector) of a FUTURE batch on a side stream, so that it runs under
        the current step's decoder work; the step that later receives this batch picks the result up (Backbone.video_tokens).
        Full fine-tune: the connector trains, so only the CLIP tower runs ahead.  Called by DevicePrefetcher for batch i+1
        before step i is issued."""
        if "vision" not in batch or not batch["vision"].is_cuda:
            return
        # Deferred: the next training_step launches it right behind its forward pass, so the side stream runs under the BACKWARD
        # pass (the skinny LoRA kernels and the GEMM tails leave CUs idle there; the forward's GEMMs do not, and the bench's
        # dominant-kernel timing stays undisturbed).  A batch whose own step comes first is computed in line by that step.
        self.backbone.defer_video_tokens(batch["vision"], ready_event, tower_only=self.full is not None)

    def discard_prefetched_vision(self, batch=None):
        """A batch announced through prefetch_vision will not be consumed (``None``: none of the announced ones will)."""
        vis = None if batch is None else batch.get("vision")
        if batch is None or torch.is_tensor(vis):
            self.backbone.discard_video_tokens(vis)

    def training_step(self, batch):
        """reference :259-306.  Leaves gradients in ``.grad`` of the trainable masters."""
        self.train(True)
        self._step += 1
        if self.lora is not None:
            self.lora.rank = self.rank
        # accumulate_grad_batches = k: micro-batch j of a window contributes (1/k) d(mse_j + l2)/dtheta - the ridge penalty counts
        # once per optimiser step, as k backward passes of loss/k give.  Everything behind the head is linear in dhidden, so the
        # head backward's two scales are the only place the 1/k enters.  (k = 1: scale 1/world, no accumulator, as ever.)
        k = self.accumulate_grad_batches
        opt = getattr(self, "optimizer", None)
        j = last = None
        if k > 1:
            if opt is None:
                raise RuntimeError("accumulate_grad_batches > 1 needs configure_optimizers() first: the optimiser owns the accumulator")
            self.check_accumulation_supported(k)
            if opt.step_count != self._window_opt_step:           # an optimiser step closed the previous window
                self._micro, self._window_opt_step = 0, opt.step_count
            j = self._micro
            if j >= k:
                raise RuntimeError(f"training_step #{j + 1} of a window of accumulate_grad_batches={k}: optimizer.step() is due")
            last = (j + 1 == k) if self.last_micro_batch is None else bool(self.last_micro_batch)
            opt.begin_micro_batch(j, last)
        self.last_micro_batch = None
        pred, y, terms = self._common_step(batch, train=True)
        self.backbone.launch_deferred_video_tokens()         # a future batch's frozen vision side: behind this forward, under this backward
        need_dh = self.lora is not None or self.full is not None
        scale = 1.0 / (self.world_size * k)
        tapped = self.head.readout_layers is not None
        if tapped:          # cached or not: the head's gradients on the mixed features, then the mix's own (and alpha_k * draw)
            self.head.backward_tapped(loss_scale=scale, l2_scale=scale)
            dh = None
        elif self._cached_step:
            self.head.backward_cached(loss_scale=scale, l2_scale=scale)
            dh = None
        else:
            dh = self.head.backward(need_dhidden=need_dh, loss_scale=scale, l2_scale=scale)
        if self.lora is not None and tapped:
            self.lora.backward(self.backbone, None, head=self.head)      # d hidden enters at the taps
        elif self.lora is not None:
            self.lora.backward(self.backbone, dh)
        elif self.full is not None:
            self.full.backward(dh)
        if k > 1:
            opt.accumulate(j, last)
            self._micro, self._window_closed = j + 1, last
        self._attach_gradients()
        self.log("train/brain_loss", terms[2])           # the objective being trained (config.loss) + l2
        if self.head.loss_kind or self.head.tw is not None:
            # the plain MSE, which the ridge forward sums anyway; with target weights the weighted one, mean_b m_b
            self.log("train/brain_mse", self.head.loss_aux[0])
        if _LP is None:
            return terms[2]          # no Lightning in this process: the plain loss value, as the built-in runner reads it
        # a scalar Lightning's automatic optimisation can call .backward() on (see _ExplicitLoss)
        return _ExplicitLoss.apply(terms[2], self, *self.parameters())

    def validation_step(self, batch):
        """reference :309-342."""
        was = self.training
        self.train(False)
        pred, y, terms = self._common_step(batch, train=False)
        self.backbone.launch_deferred_video_tokens()
        self.train(was)
        loss = terms[2].clone()
        self.log("val/brain_loss", loss)
        if self.head.loss_kind or self.head.tw is not None:
            self.log("val/brain_mse", self.head.loss_aux[0].clone())
        out = {"loss": loss, "brain_preds": pred.clone(), "brain_vals": y}
        if "subject" in batch:            # per-subject validation correlations (LogValAccuracyCallback)
            out["subject"] = torch.as_tensor(batch["subject"]).detach().cpu().to(torch.int64)
        return out

    # ------------------------------------------------------------------ evaluation pass
    def on_test_epoch_start(self):
        """Lightning hook: a fresh ``TargetScores`` (target weights' mask as the keep mask); with ``ema_decay`` and ``ema_eval``
        the whole pass runs inside ``averaged_weights()``, as a validation epoch does."""
        from .evaluate import TargetScores
        cfg = self.config
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError(f"the evaluation pass with WORLD_SIZE={os.environ['WORLD_SIZE']}: scoring is single-process only "
                             "(clips must arrive in dataset order); run one process")
        self.test_scores = TargetScores(cfg.num_target, getattr(cfg, "subjects", None), self.target_weight_mask(),
                                        getattr(cfg, "score_block", 128), self.device,
                                        save_predictions=bool(getattr(cfg, "score_save_predictions", False)))
        self.test_scores_result = None
        self._test_loss, self._test_batches = None, 0
        if self.__dict__.get("_ema_test_ctx") is None and self._ema_buffer() is not None and getattr(cfg, "ema_eval", False):
            self._ema_test_ctx = self.averaged_weights()
            self._ema_test_ctx.__enter__()

    def test_step(self, batch):
        """``validation_step`` on a clip of the evaluation split: the same eval-mode forward (the feature cache is not
        consulted), ``test/brain_loss``, and the clip's predictions and targets into ``self.test_scores``."""
        if self.__dict__.get("test_scores") is None:
            self.on_test_epoch_start()
        if "timeseries" not in batch:
            raise ValueError("test_step: the batch has no \"timeseries\": scoring needs targets (pure prediction is out of scope)")
        was = self.training
        self.train(False)
        pred, y, terms = self._common_step(batch, train=False, use_cache=False)
        self.backbone.launch_deferred_video_tokens()
        self.train(was)
        loss = terms[2].clone()
        self.log("test/brain_loss", loss)
        out = {"loss": loss, "brain_preds": pred.clone(), "brain_vals": y}
        if "subject" in batch:
            out["subject"] = torch.as_tensor(batch["subject"]).detach().cpu().to(torch.int64)
        self.test_scores.add(out["brain_preds"], y, out.get("subject"), batch.get("index"))
        self._test_loss = loss.double() if self._test_loss is None else self._test_loss + loss.double()
        self._test_batches += 1
        return out

    def on_test_epoch_end(self):
        """Leaves the EMA context, finishes the scores (``self.test_scores_result``) and logs ``test/brain_loss`` (the mean of the
        batches'), ``test_corr_avg``, ``test_r2_avg`` and ``test/brain_mse`` - with ``subjects`` also ``<key>/<subject>`` for every
        subject that had clips, the plain key being the mean over those (as ``val_corr_avg``)."""
        ctx, self._ema_test_ctx = self.__dict__.get("_ema_test_ctx"), None
        if ctx is not None:
            ctx.__exit__(None, None, None)
        cfg = self.config
        scores = self.__dict__.get("test_scores")
        if scores is None:
            return
        res = scores.finish(getattr(cfg, "score_bootstrap", 0), getattr(cfg, "score_bootstrap_seed", 0))
        self.test_scores_result = res
        if self._test_batches:
            self.log("test/brain_loss", float(self._test_loss) / self._test_batches)
        keys = ("test_corr_avg", "test_r2_avg", "test/brain_mse")
        had = [g for g in range(scores.H) if scores.counts[g] > 0]
        if scores.subjects is not None:
            for g in had:
                for k, a in zip(keys, res["avg"][g]):
                    self.log(f"{k}/{scores.subjects[g]}", float(a))
        if had:
            for i, k in enumerate(keys):
                self.log(k, float(sum(res["avg"][g][i] for g in had) / len(had)))

    # ------------------------------------------------------------------ hooks Lightning's fit loop calls (reference train.py:41-56)
    def configure_gradient_clipping(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
        """``Trainer(gradient_clip_val=1)`` (config/experiment/*.yaml:46): the global-norm clip is fused into the AdamW kernel
        (device-side norm, no host sync), so the hook only hands the threshold to the optimiser."""
        if gradient_clip_algorithm not in (None, "norm"):
            raise ValueError(f"gradient_clip_algorithm={gradient_clip_algorithm!r}: the fused optimiser clips by global norm")
        opt = getattr(optimizer, "optimizer", optimizer)            # LightningOptimizer wraps the real one
        opt.max_norm = float(gradient_clip_val or 0.0)

    def transfer_batch_to_device(self, batch, device, dataloader_idx=0):
        """Pixels / targets / weights go to the GPU; the token ids and ``padvals`` (20 KB) stay on the host so the step can size
        its unpadded row layout without a device sync (the step uploads them itself); so do a feature-cache ``index`` and the
        per-clip ``subject`` index (checked on the host, uploaded by the head)."""
        keep = ("language", "padvals", "index", "subject")
        return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) and k not in keep else v) for k, v in batch.items()}

    def on_fit_start(self):
        """Called by a Lightning ``Trainer.fit`` (never by the built-in runner).  What the bridge does not support is
        refused here instead of producing wrong gradients: anything but ONE device - Lightning's DDP / FSDP wrappers reduce
        autograd gradients, and the kernels' gradients never flow through autograd (``_ExplicitLoss.backward`` returns
        None); multi-GPU runs use the built-in runner's clip-sharded data parallelism (``torchrun ... train.py``,
        parallel.attach_data_parallel).  ``accumulate_grad_batches = k`` is supported: the module reads k from the Trainer,
        scales and accumulates inside ``training_step``, and ``_ExplicitLoss.backward`` insists on Lightning's ``loss / k``.
        (An epoch's short last window is stepped correctly too; without a notice that it closes, the optimiser runs its
        norm pass separately instead of fused into the last accumulation.)"""
        tr = self.__dict__.get("_trainer") or self.__dict__.get("trainer")
        check_accumulate_grad_batches(getattr(tr, "accumulate_grad_batches", 1) or 1)
        world = getattr(tr, "world_size", 1) or 1
        strategy = type(getattr(tr, "strategy", None)).__name__
        if world > 1 or strategy not in ("NoneType", "SingleDeviceStrategy"):
            raise ValueError(f"lightning.pytorch.Trainer with world_size={world}, strategy={strategy}: the Lightning bridge drives "
                             "ONE device.  For N GPUs launch `torchrun --nproc-per-node N train.py ...` with VLB_TRAINER=builtin "
                             "(the default): gradients are reduce-scattered by the package's own data-parallel step")

    def on_save_checkpoint(self, checkpoint: dict) -> None:
        """Lightning hook: the counter-based dropout state (head step, LoRA step) next to ``state_dict`` /
        ``optimizer_states`` (VlbAdamW.state_dict carries moments, step count and the full fine-tune's backbone masters)."""
        checkpoint["vlb_rng"] = self.rng_state()
        if "_ridge_cv_lambda" in self.__dict__:      # ridge_lambda_grid: the l2_lambda the closed-form fit chose (§5.3.6)
            checkpoint["vlb_ridge_l2_lambda"] = float(self.__dict__["_ridge_cv_lambda"])
        if "_ridge_lambda_rows" in self.__dict__:    # ridge_lambda_per_target: the penalty of every row (§5.3.7)
            checkpoint["vlb_ridge_l2_lambda_rows"] = self.__dict__["_ridge_lambda_rows"].clone()
        if "_target_weights" in self.__dict__:       # per-target loss weights / masks (§5.3.8), [max(1,G), num_target]
            checkpoint["vlb_target_weights"] = self.__dict__["_target_weights"].clone()

    def on_load_checkpoint(self, checkpoint: dict) -> None:
        if "vlb_rng" in checkpoint:
            self.set_rng_state(checkpoint["vlb_rng"])
        if "vlb_ridge_l2_lambda" in checkpoint:
            self._ridge_cv_lambda = float(checkpoint["vlb_ridge_l2_lambda"])
            if getattr(self, "head", None) is not None:
                self.head.l2_lambda = self._ridge_cv_lambda
        if "vlb_ridge_l2_lambda_rows" in checkpoint:
            self._ridge_lambda_rows = checkpoint["vlb_ridge_l2_lambda_rows"].detach().to("cpu", torch.float32).clone()
            if getattr(self, "head", None) is not None:
                self.head.set_l2_lambda_rows(self._ridge_lambda_rows.to(self.head.dev))
        if "vlb_target_weights" in checkpoint:
            tw = checkpoint["vlb_target_weights"].detach().to("cpu", torch.float32).clone()
            path = getattr(self.config, "target_weights", None)
            if path is not None:             # a configured file must hold the numbers the run was trained with
                have = self.__dict__.get("_target_weights")
                self._check_same_weights(have if have is not None else load_target_weights(
                    path, self.config.num_target, getattr(self.config, "subjects", None)), tw, path)
            self.set_target_weights(tw)

    def state_dict(self, *args, **kwargs):
        """Trainables only, upstream / peft names (what a Lightning ModelCheckpoint stores for this module; the reference saves
        the whole frozen 7B and notes the TODO, train.py:60)."""
        if getattr(self, "nnmodule", None) is None:
            return {}
        return self.trainable_state_dict()

    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        self.load_trainable_state_dict(state_dict)

    # ------------------------------------------------------------------ optimiser
    def configure_optimizers(self):
        """reference :345-379: AdamW over the trainables + CosineAnnealingLR stepped every step."""
        cfg = self.config
        from .flat import FlatTrainables
        if getattr(self, "flat", None) is None:
            self.flat = FlatTrainables(self)          # masters / bf16 copies / grads / moments -> flat buffers
        named = self.trainable_named_parameters()
        flats = [self.flat] + ([self.full.flat] if self.full is not None else [])
        groups = None
        if cfg.optimizer_groups is not None:      # per-group rates: names -> groups here, where the names exist
            assignment = assign_groups([n for n, _ in named], cfg.optimizer_groups)
            groups = (assignment, group_specs(cfg.optimizer_groups, cfg.lr, cfg.weight_decay))
        self.optimizer = VlbAdamW(named, flats, lr=cfg.lr, betas=tuple(cfg.betas), eps=cfg.eps,
                                  weight_decay=cfg.weight_decay, max_norm=cfg.gradient_clip_val, groups=groups,
                                  ema_decay=getattr(cfg, "ema_decay", None), ema_warmup=getattr(cfg, "ema_warmup", True))
        if self.lora is not None:
            self.optimizer.post_step.append(self.lora.refresh)
        if self.full is not None:
            self.optimizer.post_step.append(self.full.refresh_transposed)
        self.lr_scheduler_args = {"last_epoch": cfg.last_epoch, "T_max": cfg.t_max}
        self.scheduler = getattr(torch.optim.lr_scheduler, cfg.lr_scheduler_name)(self.optimizer, **self.lr_scheduler_args)
        return [self.optimizer], [{"scheduler": self.scheduler, "interval": "step", "frequency": 1}]


def load_safetensors_dir(path: str) -> dict:
    """Load every *.safetensors shard of a local checkpoint directory (upstream naming)."""
    from safetensors.torch import load_file
    sd = {}
    for f in sorted(os.listdir(path)):
        if f.endswith(".safetensors"):
            sd.update(load_file(os.path.join(path, f)))
    if not sd:
        raise FileNotFoundError(f"no *.safetensors under {path}")
    return sd
