"""Drop the MI355X render path into an unmodified reference checkout.

The reference's callers (train.py, eval.py, demo_script.py, sscbench/
evaluate_model_sscbench.py) import the hot path as

    from scenedino.renderer import NeRFRenderer            # renderer/__init__.py:1
    from scenedino.models import make_model                # models/__init__.py:9
    from scenedino.common.ray_sampler import ImageRaySampler

``install()`` registers this package's mirrors under those module names before the
reference is imported, so those imports resolve here while every other reference
module (encoders, data sets, trainer, losses, visualisation) stays the reference's
(``install(native_loss=True)`` also hands ``scenedino.losses.make_loss`` to this package).
``make_model`` keeps the reference's signature (scenedino/models/__init__.py:9-63): the
image encoder is this package's ``DINOv2Module`` (ViT + DPT on gfx950, one HIP graph per
pass) for every configuration it covers, else the reference's own ``make_backbone``
(models/backbones/backbone_util.py) with its ViT and DPTHead aliased to the gfx950
mirrors; the downstream head comes from ``scenedino.downstream_head.make_downstream_head``
(or, with ``install(native_head=True)``, from this package's mirror, which can be trained).
Both go to this package's BTSNet, whose parameter names equal the reference's, so
``checkpoint.pt`` state dicts load unchanged (demo_utils/utils.py:52-55).
"""
from __future__ import annotations

import importlib
import sys
import types


_NATIVE_ENCODER = True
_TRAIN_DECODER = False
_TRAIN_ENCODER = False
_NATIVE_HEAD = False
_UPSAMPLE_GT = False
_LAZY_CORR = False
_NATIVE_CRF = False


def _ref_make_model(config, downstream_config=None):
    from . import models as amd_models
    from .models.backbones import make_backbone as amd_make_backbone
    bad_decoder = None
    try:
        # the native DINOv2Module (ViT + DPT as one HIP graph; same parameter names)
        if not _NATIVE_ENCODER:
            raise NotImplementedError("native encoder disabled (install(native_encoder=False))")
        encoder = amd_make_backbone(config["encoder"],
                                    **({"upsample_gt": True} if _UPSAMPLE_GT else {}))
        if hasattr(encoder, "train_decoder"):
            encoder.train_decoder = _TRAIN_DECODER or _TRAIN_ENCODER
        if hasattr(encoder, "train_encoder"):
            encoder.train_encoder = _TRAIN_ENCODER
            from .models.backbones.dino.dpt_head import DPTHead
            if _TRAIN_ENCODER and not isinstance(encoder.decoder, DPTHead):
                bad_decoder = type(encoder.decoder).__name__
    except NotImplementedError:
        # encoder variants this build does not cover (non-DPT decoders, register / FiT3D
        # ViTs, separate gt versions, upsample-gt mode without install(upsample_gt=True)): the
        # reference's own module, whose ViT and DPTHead still resolve to the gfx950 mirrors
        # aliased by install()
        backbones = importlib.import_module("scenedino.models.backbones")
        encoder = backbones.make_backbone(config["encoder"])
    if bad_decoder is not None:
        raise NotImplementedError(
            "scenedino_amd dropin: train_encoder=True needs decoder_arch=\"dpt\" (the ViT's "
            f"differentiable path ends in the DPT decoder; this config builds {bad_decoder})")
    downstream_head = None
    if downstream_config is not None:
        if _NATIVE_HEAD:
            from .downstream_head import make_downstream_head
            downstream_head = make_downstream_head(downstream_config)
            if _LAZY_CORR and hasattr(downstream_head, "lazy_corr"):
                downstream_head.lazy_corr = True
            if _NATIVE_CRF and hasattr(downstream_head, "native_crf"):
                downstream_head.native_crf = True
        else:
            heads = importlib.import_module("scenedino.downstream_head")
            downstream_head = heads.make_downstream_head(downstream_config)
    return amd_models.make_model(config, downstream_config, encoder=encoder,
                                 downstream_head=downstream_head)


def _make_loss(config):
    """scenedino.losses.make_loss under install(native_loss=True)."""
    from . import losses as amd_losses
    if config["type"] in ("reconstruction", "stego"):
        return amd_losses.make_loss(config)
    raise ValueError(f"Unknown loss type {config['type']} (scenedino_amd dropin, native_loss=True: "
                     "'reconstruction' and 'stego')")


def install(native_encoder: bool = True, train_decoder: bool = False,
            train_encoder: bool = False, native_head: bool = False, native_loss: bool = False,
            upsample_gt: bool = False, native_crops: bool = False,
            native_metrics: bool = False, native_crf: bool = False):
    """Alias scenedino.renderer / scenedino.models.make_model / ImageRaySampler to the
    MI355X build.  Call before the first ``import scenedino...``.

    train_decoder=True (with native_encoder=True) trains the DPT decoder on the native
    kernels: a train-mode forward of the native DINOv2Module runs the frozen ViT under
    no_grad and the decoder through its differentiable path (dpt_autograd: forward GEMMs
    for the data gradients, sd_conv_wgrad for the weight gradients), so ``loss.backward()``
    reaches ``encoder.decoder.*``.  It needs a frozen ViT (``encoder_freeze: true``): the
    ViT kernels are forward-only and a training forward with trainable ViT parameters
    still raises.  Default False: DINOv2Module refuses a training forward with trainable
    encoder / decoder parameters rather than drop their gradients.

    train_encoder=True (with native_encoder=True; implies train_decoder) also trains the ViT
    on the native kernels, the reference's ``encoder_freeze: false`` recipe (trainer.py:561-573
    gives ``renderer.net.encoder.encoder.*`` its own Adam group): with a trainable
    ``encoder.*`` parameter the training forward runs the ViT through vit_autograd
    (sd_attention_bwd, sd_layernorm_bwd, sd_gelu_bwd, GEMMs on transposed packs,
    sd_conv_wgrad), so ``loss.backward()`` reaches every parameter the reference optimises.
    It needs ``decoder_arch: dpt``; any other decoder raises NotImplementedError.

    native_encoder=False keeps the image encoder entirely the reference's (its timm ViT and
    DPTHead with autograd).  The field / render path (BTSNet, NeRFRenderer, ImageRaySampler)
    is the build's either way.

    native_head=True builds this package's ``SemanticHead`` (same state-dict keys) instead of
    the reference's: its ``forward_training`` runs the downstream stage
    (``training_type: downstream_training``) on ``sd_stego_train_fwd`` / ``_bwd``,
    ``sd_cluster_probe`` and ``sd_conv_wgrad``.  Default False: the reference's head.

    native_loss=True registers a ``scenedino.losses`` module whose ``make_loss`` returns this
    package's ``ReconstructionLoss`` (``sd_recon_loss_fwd`` / ``_bwd`` on the GPU inside their
    domain, torch ops otherwise; no host sync) for ``reconstruction`` and its ``StegoLoss`` for
    ``stego``, and raises for any other type.  The reference's own losses package, which does not
    import without ``kornia``, is then never loaded.  Default False: ``scenedino.losses`` stays
    the reference's.

    native_head=True together with native_loss=True also sets ``lazy_corr = True`` on the heads
    built: ``forward_training`` then leaves a ``StegoCorrMap`` (the operand rows under the six
    correlation keys, each tensor built only when indexed) and this package's ``StegoLoss`` takes
    its fused route (``sd_stego_corr_fwd`` / ``_bwd``: no (nc, P, P) correlation tensor is
    written).  Either switch alone leaves ``lazy_corr`` False, so the reference's head or loss on
    the other side sees the eager dict of tensors.

    upsample_gt=True (with native_encoder=True) keeps ``mode: "upsample-gt"`` configurations
    (configs/model/dino_upsampler.yaml) on the native ``DINOv2Module``: its ground-truth pass
    returns per-pixel targets from this package's ``MultiScaleCropGT`` (``sd_msc_gt`` on the GPU,
    torch ops otherwise; random crops drawn on torch's RNG, not kornia's) or ``InterpolatedGT``.
    Default False: that mode falls back to the reference's backbone, which needs ``kornia``.

    native_crops=True replaces ``BTSDownstreamWrapper.sample_3d_crop``
    (scenedino/training/trainer_downstream.py:216-292) with a method of the same signature that
    calls this package's ``training.sample_3d_crop`` on ``self.renderer.net``
    (``sd_crop3d_centres`` -> ``net.query`` -> ``sd_crop3d_compact`` on the GPU, torch ops
    otherwise; one host read per call; picks and offsets drawn on torch's RNG in one call each,
    not the reference's sequence of calls; an empty depth bin drops that crop only).  A checkout
    whose trainer module does not import (ignite absent) is left as it is.  Default False: the
    reference's own method.

    native_metrics=True hands the evaluation metrics to this package's ``common.metrics``
    (``sd_depth_metrics``, ``sd_dino_metrics``, ``sd_seg_confusion`` on the GPU inside their
    domain, torch ops otherwise; no host read).  Where ``scenedino.common.metrics`` imports, its
    ``compute_depth_metrics``, ``compute_dino_metrics``, ``compute_seg_metrics`` and
    ``compute_stego_metrics`` are replaced (scenedino/evaluation/wrapper.py looks them up through
    the module at call time) and ``SegmentationMetric._calculate_pseudo_label_assignment`` becomes
    this package's ``linear_sum_assignment`` form, so ``pulp`` is not called.  Where it does not
    import (``ignite``, ``skimage`` or ``pulp`` absent), a ``scenedino.common.metrics`` module is
    registered with those functions, ``l2_scaling`` / ``median_scaling`` and the ignite-free
    ``DictMeanMetric`` / ``SegmentationMetric`` (``reset`` / ``update`` / ``compute``) under the
    reference's names.  The reference's ``base_trainer`` and ``base_evaluator`` still need ignite
    for their engines; a loop without ignite drives the aggregators itself.  Default False.

    native_crf=True sets ``native_crf = True`` on the native ``SemanticHead``s built (with
    native_head=True), so a configuration with ``apply_crf: true`` adds the ``<name>_crf`` results
    from this package's dense CRF (``sd_dense_crf`` on the GPU inside its domain, a float64 torch
    route otherwise; exact pair sums, parity with pydensecrf's lattice approximation unpinned)
    instead of raising.  Where the reference's ``scenedino.downstream_head.crf`` does not import
    (pydensecrf absent), a module of that name exporting this package's ``dense_crf`` (same
    signature, a (c, H, W) numpy array) is registered.  Default False."""
    global _NATIVE_ENCODER, _TRAIN_DECODER, _TRAIN_ENCODER, _NATIVE_HEAD, _UPSAMPLE_GT, _LAZY_CORR
    global _NATIVE_CRF
    _NATIVE_CRF = bool(native_crf)
    _UPSAMPLE_GT = bool(upsample_gt)
    _LAZY_CORR = bool(native_head and native_loss)
    _NATIVE_HEAD = bool(native_head)
    _NATIVE_ENCODER = bool(native_encoder)
    _TRAIN_DECODER = bool(train_decoder)
    _TRAIN_ENCODER = bool(train_encoder)
    from . import renderer as amd_renderer
    from .common import ray_sampler as amd_rs
    from .models import bts as amd_bts

    ren = types.ModuleType("scenedino.renderer")
    ren.NeRFRenderer = amd_renderer.NeRFRenderer
    ren.__path__ = []  # package: scenedino.renderer.nerf resolves below
    sys.modules["scenedino.renderer"] = ren
    sys.modules["scenedino.renderer.nerf"] = importlib.import_module(
        "scenedino_amd.renderer.nerf")

    models = importlib.import_module("scenedino.models")
    models.make_model = _ref_make_model
    models.BTSNet = amd_bts.BTSNet
    sys.modules["scenedino.models.bts"] = amd_bts

    rs = importlib.import_module("scenedino.common.ray_sampler")
    rs.ImageRaySampler = amd_rs.ImageRaySampler

    if native_loss:
        from . import losses as amd_losses
        lo = types.ModuleType("scenedino.losses")
        lo.make_loss = _make_loss
        lo.ReconstructionLoss = amd_losses.ReconstructionLoss
        lo.StegoLoss = amd_losses.StegoLoss
        # a bare package module: the checkout's losses/__init__.py (which imports the
        # kornia-bound module) never runs, its other files (base_loss.py, which the trainers
        # import for a type hint) still resolve
        import os
        pkg = importlib.import_module("scenedino")
        lo.__path__ = [os.path.join(p, "losses") for p in getattr(pkg, "__path__", [])]
        sys.modules["scenedino.losses"] = lo

    # The DINO / DINOv2 ViT of the encoder (dinov2_module.py:19-28 build_encoder looks
    # DINOv2Encoder up at call time): same parameter names (model.vit.*), gfx950 kernels,
    # no hub download -- the weights come from checkpoint.pt.  The DPT decoder, the
    # downsampler and the dimension reduction stay the reference's modules (BTSNet reads
    # dim_reduction's parameters for the fused sd_seg_query head).
    try:
        dm = importlib.import_module("scenedino.models.backbones.dino.dinov2_module") \
            if native_encoder else None
    except ImportError:  # the reference's encoder dependencies (timm, torchvision) absent
        dm = None
    if dm is not None:
        from .models.backbones.dino import vit as amd_vit
        from .models.backbones.dino import dpt_head as amd_dpt
        dm.DINOv2Encoder = amd_vit.DINOv2Encoder
        # build_decoder (dinov2_module.py:31-56) looks DPTHead up at call time too
        dm.DPTHead = amd_dpt.DPTHead

    if native_crops:
        try:
            td = importlib.import_module("scenedino.training.trainer_downstream")
        except ImportError:  # the trainer's dependencies (ignite) or the module itself absent
            td = None
        if td is not None:
            td.BTSDownstreamWrapper.sample_3d_crop = _sample_3d_crop

    if native_metrics:
        _install_metrics()

    if native_crf:
        _install_crf()


_METRIC_FUNCTIONS = ("compute_depth_metrics", "compute_dino_metrics", "compute_seg_metrics",
                     "compute_stego_metrics")


def _pseudo_label_assignment(self, metric_matrix):
    """SegmentationMetric._calculate_pseudo_label_assignment under install(native_metrics=True)."""
    from .common.metrics import pseudo_label_assignment
    return pseudo_label_assignment(metric_matrix)


def _install_metrics():
    from .common import metrics as amd_metrics
    try:
        cm = importlib.import_module("scenedino.common.metrics")
    except ImportError:  # the module's dependencies (ignite, skimage, pulp) absent
        cm = None
    if cm is not None:
        for name in _METRIC_FUNCTIONS:
            setattr(cm, name, getattr(amd_metrics, name))
        cm.SegmentationMetric._calculate_pseudo_label_assignment = _pseudo_label_assignment
        return
    cm = types.ModuleType("scenedino.common.metrics")
    cm.__doc__ = "scenedino_amd.common.metrics under the reference's names (dropin.install)."
    for name in _METRIC_FUNCTIONS + ("l2_scaling", "median_scaling", "DictMeanMetric",
                                     "SegmentationMetric", "NotComputableError"):
        setattr(cm, name, getattr(amd_metrics, name))
    sys.modules["scenedino.common.metrics"] = cm
    try:
        importlib.import_module("scenedino.common").metrics = cm
    except ImportError:
        pass


def _install_crf():
    from .downstream_head import crf as amd_crf
    try:
        importlib.import_module("scenedino.downstream_head.crf")
        return  # the reference's own module imports (pydensecrf present): left as it is
    except ImportError:
        pass
    cm = types.ModuleType("scenedino.downstream_head.crf")
    cm.__doc__ = "scenedino_amd.downstream_head.crf under the reference's name (dropin.install)."
    for name in ("dense_crf", "MAX_ITER", "POS_W", "POS_XY_STD", "Bi_W", "Bi_XY_STD", "Bi_RGB_STD"):
        setattr(cm, name, getattr(amd_crf, name))
    sys.modules["scenedino.downstream_head.crf"] = cm


def _sample_3d_crop(self, poses, projs, depth, z_far=100, n_crops=5, n_samples=576,
                    sample_radius=0.5, sigma_threshold=0.5):
    """BTSDownstreamWrapper.sample_3d_crop under install(native_crops=True)."""
    from .training import sample_3d_crop
    return sample_3d_crop(self.renderer.net, poses, projs, depth, z_far=z_far, n_crops=n_crops,
                          n_samples=n_samples, sample_radius=sample_radius,
                          sigma_threshold=sigma_threshold)
