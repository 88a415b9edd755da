"""Synthetic MNIST-like data with on-device upscaling."""
from .synthetic import MNIST_TRAIN_SIZE, DeviceUpsampleLoader, RandomAffine, SyntheticMNIST, synthetic_batch

__all__ = ["SyntheticMNIST", "DeviceUpsampleLoader", "RandomAffine", "synthetic_batch", "MNIST_TRAIN_SIZE"]
