from ..schedules import flowmatch_tables, get_scheduler  # noqa: F401
from .optim_config import optimizer_kwargs_from_config  # noqa: F401
from .qwen_step import QwenLoraTrainStep, map_mask_to_latent  # noqa: F401
from .flux_step import FluxKontextTrainStep  # noqa: F401
