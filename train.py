"""Drop-in for the reference's train.py (train.py:1-70): same CLI
``python train.py experiment=<name> subject=<sub-XX>`` and the same YAML keys.

The YAML is read by the built-in Hydra-subset loader (phantom_vlb_amd.config).  ``_target_: lightning.pytorch.Trainer`` and
the callbacks are served by the built-in fit loop (phantom_vlb_amd.trainer), which honours the same keys -
the default, and the loop behind every measured number and the multi-GPU path.  VLB_TRAINER=lightning opts in to the real
Lightning objects (VLBLitModule / VLBDataModule / LogValAccuracyCallback subclass the Lightning base classes whenever the
package is importable, so the reference's own unchanged train.py can drive them too): ONE device, exercised only against
tests/fake_lightning.py so far.  Comet logging is optional: without ``comet_ml`` or
credentials only the CSV logger is attached.

Root keys beyond the reference's: ``export_merged=<file>`` (merged LoRA weights) and the evaluation pass ``evaluate=test|val``,
``evaluate_out=<file.npz>``, ``ckpt_path=<file>``, ``fit=false`` (``check_evaluate_keys``).
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def export_merged(litmodule, path: str) -> str:
    """Root key ``export_merged=<file>``: after the fit a LoRA run also writes its decoder linears with the adapters merged in
    (plus the head) as one safetensors file - with the untouched rest of the base checkpoint, a plain VideoLLaMA2 decoder
    (VLBLitModule.save_merged).  The counterpart of storing only the adapters (reference train.py:60 TODO)."""
    if not getattr(litmodule.config, "use_lora", False):
        raise ValueError(f"export_merged={path!r} needs a LoRA run (litmodule.config.use_lora=true): without adapters there is "
                         "nothing to merge")
    out = litmodule.save_merged(str(path))
    print(f"[train] merged LoRA weights written to {out}")
    return out


def check_evaluate_keys(config: dict) -> tuple:
    """Root keys of the evaluation pass -> (split or None, fit, ckpt_path): ``evaluate=test|val`` scores that
    split after the fit (``evaluate_out=<file.npz>``, default ``<output_dir>/scores_<split>.npz``); ``ckpt_path=<file>`` is
    handed to ``fit``, or with ``fit=false`` - which skips the fit and needs it - to ``test``."""
    split, fit, ckpt = config.get("evaluate"), config.get("fit", True), config.get("ckpt_path")
    if split is not None and split not in ("test", "val"):
        raise ValueError(f"evaluate={split!r}: expected test or val")
    if not isinstance(fit, bool):
        raise ValueError(f"fit={fit!r}: true or false is needed")
    if not fit and not ckpt:
        raise ValueError("fit=false skips the fit and evaluates a saved run: it needs ckpt_path=<file>")
    if not fit and split is None:
        raise ValueError("fit=false without evaluate=test|val leaves nothing to do")
    if config.get("evaluate_out") and split is None:
        raise ValueError(f"evaluate_out={config['evaluate_out']!r} needs evaluate=test|val")
    if split == "test" and not config["datamodule"]["config"].get("test_lazyload_path"):
        raise ValueError("evaluate=test needs datamodule.config.test_lazyload_path (the held-out split)")
    return split, fit, (str(ckpt) if ckpt else None)


def evaluate(trainer, litmodule, datamodule, split: str, out_path: str, ckpt_path=None) -> str:
    """Score ``split`` through ``Trainer.test`` (both splits go through the same ``TargetScores``) and write the ``.npz``."""
    loader = datamodule.test_dataloader() if split == "test" else datamodule.x_dataloader(datamodule.datasets.val, shuffle=False)
    metrics = trainer.test(litmodule, dataloaders=loader, ckpt_path=ckpt_path)[0]
    out = litmodule.test_scores.write(out_path)
    print(f"[train] {split} scores written to {out}: " + ", ".join(f"{k}={v:.6g}" for k, v in sorted(metrics.items())))
    return out


def train(config: dict) -> None:
    split, do_fit, ckpt_path = check_evaluate_keys(config)            # before anything is built
    if config.get("export_merged") and not config["litmodule"]["config"].get("use_lora"):       # before the fit, not after it
        raise ValueError(f"export_merged={config['export_merged']!r} needs a LoRA run (litmodule.config.use_lora=true)")
    import torch
    from phantom_vlb_amd.config import instantiate, use_builtin_trainer
    from src import LogValAccuracyCallback
    if use_builtin_trainer():
        from phantom_vlb_amd.trainer import LearningRateMonitor, TrainableCheckpoint
    else:                                        # reference train.py:3-4,20-30: the real callbacks
        from lightning.pytorch.callbacks import LearningRateMonitor, ModelCheckpoint as TrainableCheckpoint

    seed = int(config.get("random_state", 1234))
    torch.manual_seed(seed)                      # L.seed_everything(config.random_state), train.py:18
    import numpy as np
    import random
    np.random.seed(seed)
    random.seed(seed)

    callbacks = [
        TrainableCheckpoint(monitor="val/brain_loss", filename="best_brainloss_{epoch}-{step}", mode="min",     # train.py:21-27
                            dirpath=config["output_dir"], save_last=True),
        LearningRateMonitor(logging_interval="epoch"),
        LogValAccuracyCallback(),
    ]
    loggers = []
    comet_cfg = config.get("comet_logger")
    if comet_cfg and not any(u.startswith("my_") for u in config.get("_unresolved", [])):
        try:
            loggers.append(instantiate(comet_cfg))
        except Exception as e:            # no comet_ml / no network: CSV only
            print(f"[train] comet logger unavailable ({type(e).__name__}); continuing with CSV only")
    loggers.append(instantiate(config["cvs_logger"]))

    trainer = instantiate(config["trainer"], logger=loggers, callbacks=callbacks)
    datamodule = instantiate(config["datamodule"])
    print("[train] datasets:", datamodule.datasets.dset_names)
    litmodule = instantiate(config["litmodule"])
    if getattr(datamodule.datasets, "test_names", None):
        print("[train] test split:", datamodule.datasets.test_names)
    if do_fit:
        trainer.fit(model=litmodule, datamodule=datamodule, **({"ckpt_path": ckpt_path} if ckpt_path else {}))
        trainer.save_checkpoint(config["output_dir"])          # reference train.py:58 -> <output_dir>/final.ckpt
    if split is not None:
        out_path = config.get("evaluate_out") or os.path.join(config["output_dir"], f"scores_{split}.npz")
        evaluate(trainer, litmodule, datamodule, split, out_path, None if do_fit else ckpt_path)
    if config.get("export_merged"):
        export_merged(litmodule, config["export_merged"])


if __name__ == "__main__":
    from phantom_vlb_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, "config"), sys.argv[1:])
    train(cfg)
