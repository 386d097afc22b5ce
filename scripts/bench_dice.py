"""``bench.py`` with the soft-Dice term on: the same arguments and the same JSON line, measured on a
config whose ``dice_weight`` is set (default 1; ``DDLPC_DICE_WEIGHT``) — docs/PERF.md, "Soft-Dice
term".  One process (``--gpus 1``); run from the repository root:

    python scripts/bench_dice.py --gpus 1 --steps 30 --warmup 10

Fails if the run did not take the Dice head.
"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ddlpc.train.trainer as trainer  # noqa: E402

_init = trainer.Trainer.__init__
_trainers = []


def _init_with_dice(self, cfg, *args, **kwargs):
    cfg.dice_weight = float(os.environ.get("DDLPC_DICE_WEIGHT", "1"))
    _init(self, cfg, *args, **kwargs)
    _trainers.append(self)


trainer.Trainer.__init__ = _init_with_dice
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
finally:
    # the figure is a Dice figure only if the timed steps ran the Dice head
    assert _trainers and all(t.model.dice_terms() is not None for t in _trainers), \
        "bench.py did not run the soft-Dice head: the figure above is not a Dice-on figure"
