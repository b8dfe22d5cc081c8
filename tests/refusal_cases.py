"""The render-path operators and the two bilateral solve operators as refusal test cases, shared by tests/test_meta_refusals.py (meta and
fake tensors, no GPU) and tests/test_gpu_refusals.py (device tensors): per operator a builder of valid arguments, the shapes and dtypes
of its outputs, and a list of mutations of the arguments with the message each must raise -- from the device kernel and from the Meta
kernel alike, which share one check function per operator.

Shapes: the smallest that still tell the dimensions apart -- bn = 2 images, K = 2 lobes, an env grid of R x C = 3 x 5, BRDF maps at
6 x 10 (the 2x-pooled form), a direction grid of 8 x 16; the bilateral solver on an 8 x 12 image."""
import torch
import torch.nn.functional as F

bn, K, R, C, h, w, eh, ew = 2, 2, 3, 5, 6, 10, 8, 16
BH, BW = 8, 12
CAM = [0.0, 0.0, 0.0]
F32, F64 = torch.float32, torch.float64


def uni(*shape, seed, lo=0.1, hi=0.9):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def unit(*shape, seed, dim):
    return F.normalize(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), dim=dim)


# ---- the valid arguments, drawn on the CPU --------------------------------------------------------------------------------------------
def sg():
    return [unit(bn, K, 3, R, C, seed=1, dim=2), uni(bn, K, R, C, seed=2), uni(bn, 3 * K, R, C, seed=3)]


def brdf():
    return [uni(bn, 3, h, w, seed=4), unit(bn, 3, h, w, seed=5, dim=1), uni(bn, 1, h, w, seed=6)]


def env(seed=7):
    return uni(bn, 3, R, C, eh, ew, seed=seed)


def img(seed, c=3):
    return uni(bn, c, R, C, seed=seed)


def bilateral_maps(device):
    """guide image, target, confidence and the seven grid tensors the grid operator builds for the image (a grid of arbitrary integers
    would index out of bounds in the solve kernels of a valid call)"""
    image, pred, conf = uni(bn, 3, BH, BW, seed=40).to(device), uni(bn, 1, BH, BW, seed=41).to(device), uni(bn, 1, BH, BW, seed=42).to(device)
    grid = list(torch.ops.sgrender.bilateral_grid(image, 8.0, 2.0, 8.0))      # mode 2 of BILATERAL_MODES
    return grid, pred, conf


class Op:
    """``torch.ops.sgrender.<name>(*build(device))`` is a valid call returning tensors of ``outputs`` = [(shape, dtype), ...];
    ``mutations``: (label, change of the argument list, the message the refusal carries); ``as_given``: see :meth:`build_strided`"""

    def __init__(self, name, build, outputs, mutations, as_given=()):
        self.name, self._build, self.outputs, self.mutations, self.as_given, self._built = name, build, outputs, mutations, tuple(as_given), {}

    def build(self, device):
        """the valid arguments on ``device``: built once, nothing changes them (a mutation replaces entries of the list it is given)"""
        if device not in self._built:
            self._built[device] = [a.to(device) if isinstance(a, torch.Tensor) else a for a in self._build(device)]
        return list(self._built[device])

    def build_strided(self, device):
        """the same values in non-contiguous tensors -- channels-last where 4-D, else a view with a stride of 2 in the last dimension --
        except the arguments ``as_given``, which the operator takes only contiguous"""
        def strided(t):
            if t.dim() == 4:
                return t.contiguous(memory_format=torch.channels_last)
            return torch.stack([t, t], dim=-1)[..., 0] if t.dim() else t
        return [strided(a) if isinstance(a, torch.Tensor) and i not in self.as_given else a for i, a in enumerate(self.build(device))]

    def call(self, args):
        out = getattr(torch.ops.sgrender, self.name)(*args)
        return (out,) if isinstance(out, torch.Tensor) else tuple(out)


# ---- changes of an argument list ------------------------------------------------------------------------------------------------------
def shape(i, *new):
    """argument i with another shape (same dtype and device)"""
    def f(a):
        a[i] = a[i].new_zeros(new)
    return f


def drop_dim(i):
    def f(a):
        a[i] = a[i][0]
    return f


def bf16(i):
    def f(a):
        a[i] = a[i].to(torch.bfloat16)
    return f


def dtype(i, dt):
    def f(a):
        a[i] = a[i].to(dt)
    return f


def batch(n, *idx):
    """arguments idx with a batch of n (their other dimensions kept)"""
    def f(a):
        for i in idx:
            a[i] = a[i].new_zeros((n,) + tuple(a[i].shape[1:]))
    return f


def empty_batch(a):
    """every tensor argument with a batch of 0"""
    for i, t in enumerate(a):
        if isinstance(t, torch.Tensor):
            a[i] = t[:0]


def value(i, v):
    def f(a):
        a[i] = v
    return f


def strided(i):
    """argument i as every second element of a tensor twice as long"""
    def f(a):
        a[i] = a[i].new_zeros(2 * a[i].numel())[::2]
    return f


FP32 = "fp32 tensors required"
AXIS, LAMB, WEIGHT, ZERO_SG = "axis must be [bn,SGNum,3,envRow,envCol]", "lamb must be [bn,SGNum,envRow,envCol]", "weight must be [bn,3*SGNum,envRow,envCol]", "zero-sized SG tensors"
ALBEDO, NORMAL, ROUGH, ZERO_BRDF = "diffusePred must be [bn,3,h,w]", "normalPred must be [", "roughPred must be [", "zero-sized BRDF maps"
ENV_CT, COT = "the env cotangent must be [bn,3,envRow,envCol,envHeight,envWidth]", "cotangents must be [bn,3,envRow,envCol]"
IM_SEG = "im must be [bn,3,h,w] and seg [bn,1,h,w]"
HEADS, HEADS_SHAPES = "light_heads takes the three decoders'", "light_heads shapes disagree"
ENC_IN = "light_encoder_input takes im/albedo/normal [bn,3,h,w] and rough/depth [bn,1,h,w]"
GRID_SHAPES, GRID_INT, GRID_F64 = "bilateral grid tensors of inconsistent shapes", "bilateral grid index tensors must be contiguous int32", "bilateral grid m / n must be contiguous fp64"


def sg_mutations(i):
    """of the SG trio at arguments i, i + 1, i + 2"""
    return [("axis-rank", drop_dim(i), AXIS), ("axis-xyz", shape(i, bn, K, 2, R, C), AXIS), ("lamb-lobes", shape(i + 1, bn, K + 1, R, C), LAMB),
            ("lamb-batch", batch(3, i + 1), LAMB), ("weight-channels", shape(i + 2, bn, K, R, C), WEIGHT), ("axis-bf16", bf16(i), FP32), ("weight-bf16", bf16(i + 2), FP32)]


def brdf_mutations(i):
    """of the BRDF maps at arguments i, i + 1, i + 2"""
    return [("albedo-rank", drop_dim(i), ALBEDO), ("albedo-channels", shape(i, bn, 1, h, w), ALBEDO), ("normal-size", shape(i + 1, bn, 3, h, w + 1), NORMAL),
            ("rough-channels", shape(i + 2, bn, 3, h, w), ROUGH), ("rough-batch", batch(3, i + 2), ROUGH), ("normal-bf16", bf16(i + 1), FP32)]


def lobes33(a):
    a[0], a[1], a[2] = a[0].new_zeros(bn, 33, 3, R, C), a[1].new_zeros(bn, 33, R, C), a[2].new_zeros(bn, 99, R, C)


def grid_of_another_image(a):
    """all seven grid tensors consistent, for one pixel fewer than the target has"""
    for i in (0, 1, 2, 3, 5, 6):      # nvert (4) is per image
        a[i] = a[i][:, :-1].contiguous()


def solve_mutations(pred, conf):
    """of the grid (arguments 0..6) and the target / confidence of the bilateral solve operators"""
    return [("pix2vert-rank", drop_dim(0), "pix2vert must be [B,H*W]"), ("perm-length", shape(1, bn, BH * BW - 1), GRID_SHAPES), ("nbr-fan", shape(3, bn, BH * BW, 9), GRID_SHAPES),
            ("nvert-batch", shape(4, bn + 1), GRID_SHAPES), ("n-length", shape(6, bn, BH * BW + 1), GRID_SHAPES), ("seg-int64", dtype(2, torch.int64), GRID_INT),
            ("m-fp32", dtype(5, F32), GRID_F64), ("grid-of-another-image", grid_of_another_image, "the bilateral grid was built for another shape"),
            ("pred-channels", shape(pred, bn, 4, BH, BW), "the bilateral target must be [B,C,H,W] with C in 1..3"), ("pred-rank", drop_dim(pred), "the bilateral target must be [B,C,H,W]"),
            ("conf-channels", shape(conf, bn, 3, BH, BW), "the bilateral confidence must be ["), ("pred-bf16", bf16(pred), FP32), ("conf-bf16", bf16(conf), FP32),
            ("empty-batch", empty_batch, "zero-sized bilateral target")]


def solve_fwd_args(device):
    grid, pred, conf = bilateral_maps(device)
    return grid + [pred, conf, 300.0, 1e-5, 1e-5, 10]


def solve_bwd_args(device):
    grid, pred, conf = bilateral_maps(device)
    return grid + [uni(bn, 1, BH, BW, seed=43), pred, conf, uni(bn, BH * BW, 1, seed=44).double(), 300.0, 1e-5, 1e-5, 10]


SG_SHAPES = [((bn, K, 3, R, C), F32), ((bn, K, R, C), F32), ((bn, 3 * K, R, C), F32)]
BRDF_SHAPES = [((bn, 3, h, w), F32), ((bn, 3, h, w), F32), ((bn, 1, h, w), F32)]
RGB, ENV, NONE, SCALAR = ((bn, 3, R, C), F32), ((bn, 3, R, C, eh, ew), F32), ((0,), F32), ((), F32)

OPS = [
    Op("sg_to_env", lambda dev: sg() + [eh, ew, True, True], [ENV, SG_SHAPES[1], SG_SHAPES[2]],
       sg_mutations(0) + [("33-lobes", lobes33, "SGNum > 32 is not supported"), ("empty-batch", empty_batch, ZERO_SG)]),
    Op("sg_to_env_bwd", lambda dev: [env()] + sg() + [eh, ew, 1], SG_SHAPES,
       sg_mutations(1) + [("cotangent-grid", shape(0, bn, 3, R, C, eh, ew - 1), ENV_CT), ("cotangent-rank", drop_dim(0), ENV_CT), ("cotangent-batch", batch(3, 0), ENV_CT),
                          ("cotangent-bf16", bf16(0), FP32), ("empty-batch", empty_batch, ZERO_SG)]),
    Op("render_env", lambda dev: brdf() + [env(), 57.0, 0.05, CAM], [RGB, RGB],
       brdf_mutations(0) + [("env-rank", drop_dim(3), "envmap must be [bn,3,envRow,envCol,envHeight,envWidth]"), ("env-batch", batch(3, 3), "envmap must be ["),
                            ("env-channels", shape(3, bn, 1, R, C, eh, ew), "envmap must be ["), ("env-bf16", bf16(3), FP32), ("empty-batch", empty_batch, ZERO_BRDF)]),
    Op("render_env_bwd_env", lambda dev: [img(8), img(9)] + brdf() + [eh, ew, 57.0, 0.05, CAM], [ENV],
       brdf_mutations(2) + [("cotangent-rank", drop_dim(0), COT), ("cotangents-differ", shape(1, bn, 3, R, C + 1), COT), ("cotangent-batch", batch(3, 0, 1), COT),
                            ("cotangent-channels", shape(0, bn, 1, R, C), COT), ("cotangent-bf16", bf16(1), FP32), ("empty-batch", empty_batch, ZERO_BRDF)]),
    Op("render_bwd_brdf", lambda dev: [img(8), img(9)] + brdf() + [env(), None, None, None, eh, ew, 57.0, 0.05, CAM, False], BRDF_SHAPES,
       brdf_mutations(2) + [("no-light", value(5, None), "render_bwd_brdf needs the env image or the SG parameters"), ("cotangent-rank", drop_dim(0), COT),
                            ("cotangents-differ", shape(1, bn, 3, R + 1, C), COT), ("cotangent-batch", batch(3, 0, 1), COT), ("env-bf16", bf16(5), FP32),
                            ("cotangent-bf16", bf16(0), FP32), ("empty-batch", empty_batch, ZERO_BRDF)]),
    Op("fused_render", lambda dev: brdf() + sg() + [eh, ew, 57.0, 0.05, CAM, 1, True, True], [ENV, RGB, RGB, SG_SHAPES[1], SG_SHAPES[2]],
       sg_mutations(3) + brdf_mutations(0) + [("maps-batch", batch(3, 0, 1, 2), "BRDF maps and SG parameters disagree on the batch size"),
                                              ("premap-2", value(11, 2), "fused_render premap must be 0 (post-tan), 1 (decoder outputs in [0, 1]) or 3 (raw decoder outputs)"),
                                              ("empty-batch", empty_batch, ZERO_SG)]),
    Op("fused_render_bwd_sg", lambda dev: [env(10), img(8), img(9)] + brdf() + sg() + [eh, ew, 57.0, 0.05, CAM, 1], SG_SHAPES,
       sg_mutations(6) + brdf_mutations(3) + [("diffuse-cotangent-grid", shape(1, bn, 3, R, C + 1), "diffuse / specular cotangents must be [bn,3,envRow,envCol]"),
                                              ("spec-cotangent-rank", drop_dim(2), "diffuse / specular cotangents must be"), ("cotangent-batch", batch(3, 1, 2), "diffuse / specular cotangents must be"),
                                              ("env-cotangent-grid", shape(0, bn, 3, R, C, eh + 1, ew), ENV_CT), ("env-cotangent-bf16", bf16(0), FP32), ("empty-batch", empty_batch, ZERO_SG)]),
    Op("lsregress_coef", lambda dev: [img(11), img(12)], [((bn,), F32)],
       [("shapes-differ", shape(1, bn, 3, R, C + 1), "LSregress needs pred and gt of one shape"), ("batch-differs", batch(3, 1), "LSregress needs pred and gt of one shape"),
        ("no-batch", lambda a: a.__setitem__(slice(0, 2), [a[0].sum(), a[1].sum()]), "LSregress needs pred and gt of one shape"), ("gt-bf16", bf16(1), FP32)]),
    Op("lsregress_diffspec_coef", lambda dev: [img(11), img(12), img(13)], [((bn, 2), F32)],
       [("spec-differs", shape(1, bn, 3, R, C + 1), "LSregressDiffSpec needs diff, spec and imOrig of one shape"), ("im-batch", batch(3, 2), "LSregressDiffSpec needs diff, spec and imOrig of one shape"),
        ("im-rank", drop_dim(2), "LSregressDiffSpec needs diff, spec and imOrig of one shape"), ("diff-bf16", bf16(0), FP32)]),
    Op("render_loss", lambda dev: [img(11), img(12), uni(bn, 3, h, w, seed=14), uni(bn, 1, h, w, seed=15), R, C, True], [SCALAR, ((1,), F32), ((2,), F32), RGB, RGB, ((bn, 1, R, C), F32), ((bn, 2), F32)],
       [("diffuse-rank", drop_dim(0), "diffuse/spec must be [bn,3,"), ("diffuse-grid", shape(0, bn, 3, R, C + 1), "diffuse/spec must be [bn,3,"),
        ("spec-differs", shape(1, bn, 1, R, C), "diffuse/spec must be [bn,3,"), ("im-rank", drop_dim(2), IM_SEG), ("im-channels", shape(2, bn, 1, h, w), IM_SEG), ("im-batch", batch(3, 2), IM_SEG),
        ("seg-size", shape(3, bn, 1, h, w - 1), IM_SEG), ("seg-bf16", bf16(3), FP32)]),
    Op("render_loss_bwd", lambda dev: [uni(1, seed=16), 1.0, uni(1, seed=17), img(11), img(12), img(13), img(14, 1), uni(bn, 2, seed=18)], [RGB, RGB],
       [("diffuse-rank", drop_dim(3), "render_loss_bwd shapes disagree"), ("spec-differs", shape(4, bn, 3, R, C + 1), "render_loss_bwd shapes disagree"),
        ("im-batch", batch(3, 5), "render_loss_bwd shapes disagree"), ("cotangent-bf16", bf16(0), FP32), ("scale-bf16", bf16(2), FP32), ("coef-bf16", bf16(7), FP32)]),
    Op("render_loss_finalize", lambda dev: [img(11), img(12), uni(2, seed=19), img(13), img(14, 1), uni(bn, 2, seed=18)], [SCALAR, ((1,), F32)],
       [("three-totals", shape(2, 3), "render_loss_finalize takes the two totals [numerator, denominator]"), ("no-totals", shape(2, 0), "render_loss_finalize takes the two totals"),
        ("parts-bf16", bf16(2), FP32), ("diffuse-bf16", bf16(0), FP32)]),
    Op("recon_loss_parts", lambda dev: [env(), env(20), img(14, 1), torch.ones(bn, 1, 1, 1), 1.0], [((2,), F32), ((bn, R * C), F32), ((bn,), F32)],
       [("env-rank", drop_dim(0), "envmapsPred / envmaps must both be [bn,3,envRow,envCol,envHeight,envWidth]"), ("gt-grid", shape(1, bn, 3, R, C, eh, ew + 1), "envmapsPred / envmaps must both be"),
        ("gt-batch", batch(3, 1), "envmapsPred / envmaps must both be"), ("channels", lambda a: a.__setitem__(slice(0, 2), [a[0][:, :1], a[1][:, :1]]), "envmapsPred / envmaps must both be"),
        ("mask-size", shape(2, bn, 1, R, C + 1), "the pooled object mask must be [bn,1,envRow,envCol] and envmapsInd [bn,...]"), ("ind-batch", batch(3, 3), "the pooled object mask must be"),
        ("ind-bf16", bf16(3), FP32)]),
    Op("recon_loss_bwd", lambda dev: [uni(1, seed=21), env(), env(20), uni(bn, R * C, seed=22), uni(bn, seed=23), 1.0], [ENV],
       [("env-rank", drop_dim(1), "recon_loss_bwd shapes disagree"), ("gt-grid", shape(2, bn, 3, R, C, eh + 1, ew), "recon_loss_bwd shapes disagree"), ("gt-batch", batch(3, 2), "recon_loss_bwd shapes disagree"),
        ("cotangent-bf16", bf16(0), FP32), ("mask-bf16", bf16(3), FP32)]),
    Op("light_heads", lambda dev: [uni(bn, 3 * K, R, C, seed=24), uni(bn, K, R, C, seed=25), uni(bn, 3 * K, R, C, seed=26), True], SG_SHAPES + [((bn, 7 * K, R, C), F32)],
       [("axis-rank", drop_dim(0), HEADS), ("lamb-rank", drop_dim(1), HEADS), ("axis-channels", shape(0, bn, 3 * K + 1, R, C), HEADS), ("lamb-lobes", shape(1, bn, K + 1, R, C), HEADS_SHAPES),
         ("weight-batch", batch(3, 2), HEADS_SHAPES), ("weight-bf16", bf16(2), FP32)]),
    Op("light_heads_bwd", lambda dev: [uni(bn, 3 * K, R, C, seed=24), uni(bn, K, R, C, seed=25), uni(bn, 3 * K, R, C, seed=26), sg()[0], sg()[1], sg()[2], None],
       [((bn, 3 * K, R, C), F32), ((bn, K, R, C), F32), ((bn, 3 * K, R, C), F32)],
       [("axis-rank", drop_dim(0), HEADS), ("axis-channels", shape(0, bn, 3 * K + 1, R, C), HEADS), ("lamb-grid", shape(1, bn, K, R, C + 1), HEADS_SHAPES), ("weight-batch", batch(3, 2), HEADS_SHAPES),
        ("cotangent-bf16", bf16(4), FP32), ("axis-bf16", bf16(0), FP32)]),
    Op("sg_shading", lambda dev: sg() + [eh, ew, 1], [RGB], sg_mutations(0) + [("empty-batch", empty_batch, ZERO_SG)]),
    Op("light_albedo_scale", lambda dev: [img(27), img(28), img(29), img(30), uni(bn, 3, h, w, seed=31)], [((4,), F32)],
       [("diffuse-differs", shape(1, bn, 3, R, C + 1), "light_albedo_scale needs four render images of one shape"), ("spec-batch", batch(3, 3), "light_albedo_scale needs four render images of one shape"),
        ("scaled-rank", drop_dim(2), "light_albedo_scale needs four render images of one shape"), ("albedo-bf16", bf16(4), FP32)]),
    Op("light_encoder_input", lambda dev: [uni(bn, 3, h, w, seed=32)] + brdf() + [uni(bn, 1, h, w, seed=33), 2 * h, 2 * w], [((bn, 11, 2 * h, 2 * w), F32), BRDF_SHAPES[0], BRDF_SHAPES[2]],
       [("im-rank", drop_dim(0), ENC_IN), ("im-channels", shape(0, bn, 1, h, w), ENC_IN), ("albedo-size", shape(1, bn, 3, h, w + 1), ENC_IN), ("normal-batch", batch(3, 2), ENC_IN),
        ("rough-channels", shape(3, bn, 3, h, w), ENC_IN), ("depth-size", shape(4, bn, 1, h + 1, w), ENC_IN), ("depth-bf16", bf16(4), FP32)]),
    Op("light_objective_stage3", lambda dev: [uni(1, seed=34).reshape(()), uni(2, seed=35), uni(4, seed=36), 1.0, 10.0, eh, ew], [SCALAR, SCALAR],
       [("three-sums", shape(2, 3), "light_objective_stage3 arguments"), ("no-numerator", shape(1, 0), "light_objective_stage3 arguments"), ("strided-sums", strided(2), "light_objective_stage3 arguments"),
        ("sums-bf16", bf16(2), FP32)], as_given=(2,)),
    Op("bilateral_solve_fwd", solve_fwd_args, [((bn, 1, BH, BW), F32), ((bn, BH * BW, 1), F64)], solve_mutations(7, 8), as_given=range(7)),
    Op("bilateral_solve_bwd", solve_bwd_args, [((bn, 1, BH, BW), F32), ((bn, 1, BH, BW), F32)],
       solve_mutations(8, 9) + [("cotangent-channels", shape(7, bn, 2, BH, BW), "the bilateral cotangent must match the target"), ("cotangent-bf16", bf16(7), "the bilateral cotangent must match the target"),
                                ("yhat-length", shape(10, bn, BH * BW - 1, 1), "yhat must be the fp64 [B,H*W,C] tensor of the forward solve"), ("yhat-fp32", dtype(10, F32), "yhat must be the fp64")], as_given=range(7)),
]
BY_NAME = {op.name: op for op in OPS}
MUTATIONS = [(op.name, label) for op in OPS for label, _, _ in op.mutations]


def mutated(op, label, device, strided=False):
    """-> (arguments with the change applied, the message)"""
    args = op.build_strided(device) if strided else op.build(device)
    change, message = next((c, m) for l, c, m in op.mutations if l == label)
    change(args)
    return args, message


def message_of(exc):
    """the refusal's own text (PyTorch may append the C++ call stack)"""
    return str(exc).split("\nException raised from")[0]
