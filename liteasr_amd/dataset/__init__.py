from .asr_dataset import AudioFileDataset  # noqa: F401
from .liteasr_dataset import LiteasrDataset  # noqa: F401
from .pretrain_dataset import RawAudioFileDataset  # noqa: F401
