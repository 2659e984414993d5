from .nets import AlexNetLPIPS, VGG19Style  # noqa: F401
