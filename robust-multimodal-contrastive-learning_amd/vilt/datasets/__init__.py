from .base_dataset import (collate, collate_uint8, collate_raw_uint8, Uint8Batch, RawUint8Batch, RawView, BaseDataset, select_from_sizes,  # noqa: F401
                           write_arrow_table)
from .nlvr2_dataset import NLVR2Dataset  # noqa: F401,E402
from .coco_caption_karpathy_dataset import CocoCaptionKarpathyDataset  # noqa: F401,E402
from .f30k_caption_karpathy_dataset import F30KCaptionKarpathyDataset  # noqa: F401,E402
from .vg_caption_dataset import VisualGenomeCaptionDataset  # noqa: F401,E402
from .sbu_caption_dataset import SBUCaptionDataset  # noqa: F401,E402
from .conceptual_caption_dataset import ConceptualCaptionDataset  # noqa: F401,E402
from .vqav2_dataset import VQAv2Dataset  # noqa: F401,E402
