"""Losses of the training recipes (mirror of scenedino/losses/__init__.py).  The first stage's
ReconstructionLoss stays the reference's (its terms run on this package's autograd paths);
the downstream stage's StegoLoss is provided here."""
from .stego_loss import StegoLoss


def make_loss(config):
    loss_type = config["type"]
    if loss_type == "stego":
        return StegoLoss(config)
    raise ValueError(f"Unknown loss type {loss_type} (this package provides 'stego')")


__all__ = ["StegoLoss", "make_loss"]
