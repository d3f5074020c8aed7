"""CoOp / CoCoOp / ZeroshotCLIP / IVLP / MaPLe / PromptSRC / LinearProbeCLIP / LoRA trainers (registered in
fsp_amd.engine.TRAINER_REGISTRY)."""
from . import coop, cocoop, zsclip, deep, linear_probe, lora  # noqa: F401
