"""CoOp / CoCoOp / ZeroshotCLIP / IVLP / MaPLe / PromptSRC / LinearProbeCLIP trainers (registered in
fsp_amd.engine.TRAINER_REGISTRY)."""
from . import coop, cocoop, zsclip, deep, linear_probe  # noqa: F401
