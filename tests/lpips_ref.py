"""Float64 restatement of LPIPS v0.1 / AlexNet for the tests, written from the published definition (Zhang, Isola, Efros,
Shechtman, Wang: "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric", CVPR 2018, eq. 1, with the released
model's conventions): inputs in [-1, 1], a fixed per-channel shift / scale, the five ReLU outputs of AlexNet's convolutional
part; per level every pixel's channel vector is scaled to unit length (x / (|x|_2 + 1e-10)), the squared difference is weighted
per channel by non-negative weights and averaged over the pixels; the five levels are summed.

Nothing here touches the GPU or the package's kernels: torch CPU in float64 and Pillow only."""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

EPS = 1e-10
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CONVS = ((0, 4, 2), (3, 1, 2), (6, 1, 1), (8, 1, 1), (10, 1, 1))        # (index in AlexNet.features, stride, padding)


def unit(x, dim):
    """x / (|x|_2 + eps) along `dim` (the eps outside the root)."""
    return x / (torch.sqrt((x * x).sum(dim, keepdim=True)) + EPS)


def layer(a, r, ref_index, w):
    """One level on rows: a [n, hw, C], r [m, hw, C], w [C] (any float dtype; computed in float64) -> float64 [n]."""
    a, r, w = a.double(), r.double(), w.double()
    rr = r[torch.as_tensor(ref_index, dtype=torch.long)]
    d = unit(a, -1) - unit(rr, -1)
    return (d * d * w).sum(-1).mean(-1)


def layer_scale(a, r, ref_index, w):
    """T_j = mean_p sum_c w_c (|a_hat| + |r_hat|)^2: the magnitude the rounding-error bound of a level is stated in."""
    a, r, w = a.double(), r.double(), w.double()
    rr = r[torch.as_tensor(ref_index, dtype=torch.long)]
    s = unit(a, -1).abs() + unit(rr, -1).abs()
    return (s * s * w).sum(-1).mean(-1)


def alex_features(sd, x):
    """x float64 [n, 3, h, w] (already shifted / scaled) -> the five ReLU outputs [n, C, h', w']."""
    feats = []
    for i, (idx, stride, pad) in enumerate(CONVS):
        if i in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[f"features.{idx}.weight"].double(), sd[f"features.{idx}.bias"].double(), stride=stride, padding=pad))
        feats.append(x)
    return feats


def scaling(x):
    """The released model's input layer on [-1, 1] images [n, 3, h, w]."""
    return (x - torch.tensor(SHIFT, dtype=x.dtype)[None, :, None, None]) / torch.tensor(SCALE, dtype=x.dtype)[None, :, None, None]


def lpips_alex(sd, x0, x1):
    """Images in [-1, 1], float64 [n, 3, h, w] each -> float64 [n]."""
    with torch.no_grad():
        f0, f1 = alex_features(sd, scaling(x0.double())), alex_features(sd, scaling(x1.double()))
        total = torch.zeros(x0.shape[0], dtype=torch.float64)
        for i, (a, b) in enumerate(zip(f0, f1)):
            w = sd[f"lin{i}.model.1.weight"].double().reshape(1, -1, 1, 1)
            d = unit(a, 1) - unit(b, 1)
            total += (d * d * w).sum(1).mean((1, 2))
    return total


def luma(rgb):
    """ITU-R 601-2 luma in 16-bit fixed point, as Pillow's convert("L") documents it: u8 [..., 3] -> u8 [...]."""
    v = rgb.astype(np.uint32)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def pil_input(img, resize=(256, 256), grey=True):
    """The PIL calls of the filter's pre-processing, re-issued against the installed Pillow: u8 RGB array or PIL image ->
    float64 [3, h, w] in [-1, 1]."""
    im = Image.fromarray(img) if isinstance(img, np.ndarray) else img
    im = im.convert("L").convert("RGB") if grey else im.convert("RGB")
    if resize:
        im = im.resize(resize)
    x = torch.from_numpy(np.asarray(im).astype(np.float64) / 255.0).permute(2, 0, 1)
    return x * 2.0 - 1.0


def distance(sd, original, augmented, resize=(256, 256), grey=True):
    """float: the LPIPS distance of two images (arrays, PIL images or paths) after `pil_input`."""
    def opened(v):
        return Image.open(v) if isinstance(v, (str, bytes)) or hasattr(v, "__fspath__") else v
    a, b = pil_input(opened(original), resize, grey), pil_input(opened(augmented), resize, grey)
    return float(lpips_alex(sd, a[None], b[None])[0])
