"""MI355X-native SG x microfacet render layer (drop-in for the reference's models.renderingLayer /
models.output2env call boundary; the compute lives in libsgrender.so, see include/sgrender.h)."""
from ._lib import SgrenderError, SgrenderUnavailable  # noqa: F401
from . import ops  # noqa: F401  (torch.ops.sgrender.* registration)
from .layers import light_albedo_scale, light_encoder_input, light_heads, output2env, output_radiance, predToShading, render_from_sg, renderingLayer, renderLayer, unpack_envmaps  # noqa: F401
from .bilateral import BILATERAL_MODES, BilateralLayer, bilateral_solve  # noqa: F401
from .brdf_losses import BRDFObjective, batch_ranking_loss, brdf_objective  # noqa: F401
from .brdf_inputs import brdf_encoder_input  # noqa: F401
from .brdf_heads import brdf_head, brdf_heads  # noqa: F401
from .export import EXPORT_KINDS, export_env_hwc, export_env_mosaic, export_image, export_predictions  # noqa: F401
from .loader_prep import loader_brdf_maps, loader_envmaps, loader_masks, loader_scale_hdr, prepare_batch  # noqa: F401
from .real_loader_prep import iiw_image, nyu_augmentation, nyu_prepare_batch  # noqa: F401
from .pil_resize import PIL_FILTERS, PIL_RESIZE_PATHS, iiw_geometry, iiw_resize_crop, loader_resize, pil_resize  # noqa: F401
from .eval_metrics import depth_log_rmse, iiw_judgements, normal_angle_error, whdr, whdr_from_ranking  # noqa: F401
from .gn_stage import GroupNormReLU, group_norm_relu, group_norm_relu_resize, group_norm_relu_resize_upcat, group_norm_relu_upcat  # noqa: F401
from .gn_stage import SiblingGroupNormReLU, group_norm_relu_resize_upcat_siblings, group_norm_relu_upcat_siblings  # noqa: F401
from .final_conv import FinalConv, final_conv, group_norm_relu_final_conv  # noqa: F401
from .light_final_conv import LightFinalConv, light_final_conv  # noqa: F401
from .encoder_conv import EncoderConv, encoder_conv, encoder_conv_cat  # noqa: F401
from .graphs import CapturedStep, capture_step  # noqa: F401
from .handoff import loadH5, read_cascade_handoff, write_cascade_handoff, writeH5ToFile  # noqa: F401
from .losses import (LSregress, LSregressDiffSpec, combine_loss_parts, ddp_loss_scale, disable_native_allreduce,  # noqa: F401
                     enable_native_allreduce, light_objective, light_objective_supported, native_allreduce_enabled, recon_loss, render_loss)

__all__ = ["pil_resize", "iiw_resize_crop", "iiw_geometry", "loader_resize", "PIL_FILTERS", "PIL_RESIZE_PATHS", "whdr", "whdr_from_ranking", "iiw_judgements", "normal_angle_error", "depth_log_rmse", "nyu_prepare_batch", "nyu_augmentation", "iiw_image", "export_image", "export_env_mosaic", "export_env_hwc", "export_predictions", "EXPORT_KINDS", "loader_masks", "loader_scale_hdr", "loader_brdf_maps", "loader_envmaps", "prepare_batch", "encoder_conv", "encoder_conv_cat", "EncoderConv", "light_final_conv", "LightFinalConv", "final_conv", "group_norm_relu_final_conv", "FinalConv", "group_norm_relu", "group_norm_relu_upcat", "group_norm_relu_resize", "group_norm_relu_resize_upcat", "GroupNormReLU", "group_norm_relu_upcat_siblings", "group_norm_relu_resize_upcat_siblings", "SiblingGroupNormReLU", "brdf_heads", "brdf_head", "brdf_encoder_input", "brdf_objective", "batch_ranking_loss", "BRDFObjective", "BilateralLayer", "bilateral_solve", "BILATERAL_MODES", "light_albedo_scale", "light_encoder_input", "light_heads", "unpack_envmaps", "output2env", "renderingLayer", "render_from_sg", "renderLayer", "output_radiance", "predToShading",
           "LSregress", "LSregressDiffSpec", "render_loss", "recon_loss", "combine_loss_parts", "ddp_loss_scale", "light_objective",
           "light_objective_supported", "enable_native_allreduce", "disable_native_allreduce", "native_allreduce_enabled", "capture_step", "CapturedStep", "writeH5ToFile", "loadH5", "write_cascade_handoff", "read_cascade_handoff", "SgrenderError", "SgrenderUnavailable"]
