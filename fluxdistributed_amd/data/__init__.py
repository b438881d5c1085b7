from .loader import PrefetchLoader  # noqa: F401
from .synthetic import SyntheticBatcher  # noqa: F401
from .imagenet import minibatch, minibatch_raw, train_solutions, labels, makepaths  # noqa: F401
from .preprocess import preprocess, center_crop, resize_smallest_dimension  # noqa: F401
from .preprocess import RawBatch, pack_images, preprocess_batch  # noqa: F401
