from ..convnet import ConvUnit, fold_batchnorm  # noqa: F401
from .spec import build_units, state_dict_shapes  # noqa: F401


def __getattr__(name):          # the model itself needs the GPU library's host side; the table above does not
    if name in ("InceptionV3FID", "default_weights_path", "WEIGHTS_NAME"):
        from . import inception_v3
        return getattr(inception_v3, name)
    raise AttributeError(name)
