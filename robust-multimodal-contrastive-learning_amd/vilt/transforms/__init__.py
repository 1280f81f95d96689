from .utils import MinMaxResize, min_max_resize_size, pixelbert_transform, pixelbert_uint8_transform, decode_uint8_transform, normalize_lut, keys_to_transforms  # noqa: F401
from .utils import pixelbert_randaug_transform, decode_uint8_randaug_transform  # noqa: F401
from .randaug import RandAugment, draw_plan, apply_plan_pil, plan_params  # noqa: F401
