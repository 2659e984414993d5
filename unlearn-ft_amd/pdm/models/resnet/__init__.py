from .resnet50 import ResNet50Classifier, default_weights_path  # noqa: F401
