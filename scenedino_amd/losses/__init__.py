"""Losses of the training recipes (mirror of scenedino/losses/__init__.py): the first stage's
ReconstructionLoss (fused sd_recon_loss_fwd / _bwd kernels on the GPU inside their domain, torch
ops everywhere else; losses/reconstruction_loss.py) and the downstream stage's StegoLoss."""
from .reconstruction_loss import ReconstructionLoss
from .stego_loss import StegoLoss


def make_loss(config):
    loss_type = config["type"]
    if loss_type == "reconstruction":
        return ReconstructionLoss(config)
    if loss_type == "stego":
        return StegoLoss(config)
    raise ValueError(f"Unknown loss type {loss_type} (this package provides 'reconstruction' "
                     "and 'stego')")


__all__ = ["ReconstructionLoss", "StegoLoss", "make_loss"]
