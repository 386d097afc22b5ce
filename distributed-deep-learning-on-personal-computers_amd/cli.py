"""Command-line entry point: ``python -m ddlpc {train,validate,predict,config}``.

The reference is started by hand on every PC (server first, then workers; rank from a
hostname table, ref.py:223-251) and has no flags at all.  Here one command
line serves every rank: launch it under ``torchrun`` (RANK / WORLD_SIZE / LOCAL_RANK /
MASTER_ADDR / MASTER_PORT come from the environment), e.g.

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m ddlpc train \
        --batch-per-gpu 32 --accum-steps 1 --epochs 100 --log-dir runs/x

Every ``TrainConfig`` / ``ModelConfig`` field is a ``--flag`` (``--config file.yaml`` first,
flags override).  ``train`` prints the final reduced metrics as one JSON line on rank 0;
``validate`` evaluates a checkpoint on the held-out split; ``predict`` segments whole scenes
(a file or a directory of images, any size) by overlap-tile inference, e.g.

    python -m ddlpc predict --checkpoint runs/x/ckpt_900.pt --input scenes/ --out-dir pred/

(``--tta d4`` averages every window over the eight symmetries of the square, the test-time
counterpart of ``train --augment d4``.)

``train --data scene_dir --data-dir scenes/ --augment d4`` trains on uncut scenes of unequal size
(augmented random crops cut on the device, ``data/scenes.py``), and with ``--zoom-min 0.5
--zoom-max 2 --rotate-deg 30`` the crops are zoomed and rotated at random on the way;
``--class-weights 1,1,1,1,4,4`` (one number per class) or ``--class-weights median_freq`` (from
the training split's labels) trains with ``CrossEntropyLoss(weight=...)``, fused into the head
kernels — the validation loss stays unweighted, the per-class IoU shows the effect;
``config`` prints the resolved configuration (handy for writing a YAML to start from).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import List, Optional

from .config import add_config_args, config_from_args


_PREDICT_ARGS = ("input", "out_dir", "pred_tile", "overlap", "blend", "window_batch", "save_proba",
                 "tta")


def _rank0() -> bool:
    return int(os.environ.get("RANK", "0")) == 0


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="ddlpc", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p_train = add_config_args(sub.add_parser("train", help="train a U-Net (all ranks)"))
    p_train.add_argument("--device", default=None, help="cuda[:i] | cpu (default: auto)")
    p_val = add_config_args(sub.add_parser("validate", help="evaluate on the held-out split"))
    p_val.add_argument("--checkpoint", default=None)
    p_val.add_argument("--device", default=None)
    p_pred = add_config_args(sub.add_parser("predict", help="segment whole scenes (overlap-tile)"))
    p_pred.add_argument("--checkpoint", required=True)
    p_pred.add_argument("--input", required=True, help="an image, or a directory of images "
                        "(+ optional .npy label maps)")
    p_pred.add_argument("--out-dir", required=True)
    p_pred.add_argument("--pred-tile", type=int, default=None, help="window size (default: --tile)")
    p_pred.add_argument("--overlap", type=int, default=None, help="even, <= tile/2 (default: tile/4)")
    p_pred.add_argument("--blend", choices=("core", "cosine"), default="cosine")
    p_pred.add_argument("--window-batch", type=int, default=16)
    p_pred.add_argument("--save-proba", action="store_true")
    p_pred.add_argument("--tta", choices=("none", "flip", "d4"), default="none",
                        help="test-time augmentation: average every window over 4 / 8 symmetries")
    p_pred.add_argument("--device", default=None)
    add_config_args(sub.add_parser("config", help="print the resolved config as JSON"))
    args = ap.parse_args(argv)
    cmd = args.cmd
    device = getattr(args, "device", None)
    checkpoint = getattr(args, "checkpoint", None)
    pred_args = {k: getattr(args, k, None) for k in _PREDICT_ARGS}
    for k in ("cmd", "device", "checkpoint") + _PREDICT_ARGS:
        if hasattr(args, k):
            delattr(args, k)
    cfg = config_from_args(args)
    if cmd == "config":
        print(json.dumps(cfg.to_dict(), indent=2))
        return 0
    if cmd == "predict":
        from .infer import predict
        metrics = predict(cfg, checkpoint, pred_args.pop("input"), **pred_args, device=device)
        if _rank0():
            print(json.dumps({"cmd": cmd, **metrics}))
        return 0
    from .train.trainer import train, validate
    if cmd == "train":
        metrics = train(cfg, device=device)
    else:
        metrics = validate(cfg, checkpoint=checkpoint, device=device)
    if _rank0():
        print(json.dumps({"cmd": cmd, **{k: (float(v) if isinstance(v, (int, float)) else v)
                                         for k, v in (metrics or {}).items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
