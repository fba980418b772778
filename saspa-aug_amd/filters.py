"""The filter stage that follows generation: the two models the reference runs inside
`create_json_of_image_name_to_augmented_images_paths` (all_utils/utils.py:252-255, :306-323, :357-375), as launch
sequences of the gfx950 kernels.

  * `SemanticFilter` -- OpenAI CLIP RN50 (`clip.load('RN50')`, all_utils/utils.py:253): image tower = ModifiedResNet +
    attention pool, text tower = 12-layer transformer; an augmented image passes when the dataset's positive prompt
    (`ds_utils.get_basic_prompt()`) beats the six negative prompts (:306-312, `get_semantic_filtering` :169-177).
  * `LpipsAlex` -- LPIPS v0.1 on AlexNet (`lpips.LPIPS(net='alex')`, all_utils/utils.py:269-270): an augmented image passes when
    `lpips_min <= d(original, augmented) <= lpips_max` (:377-381), both images grey, 256 x 256 (`calc_lpips_distance` :576-590).
  * `ConfidenceFilter` -- the baseline classifier WSDAN_CAL (fgvc/models/cal.py:131-228; loader
    all_utils/dataset_utils.py:87-115): passes when the SOURCE image's label is among the top-k (10) logits (:357-366); with
    `too_high` (the reference's `filter_confidence_higher_than`, :368-373) an image that passes top-k is dropped when the softmax
    probability of that label exceeds the bound.
  * `ClassFilter` -- the per-class CLIP filter of the Real-Guidance baseline (`clip_filtering="per_class"`, :272-304, :180-191,
    :383-393): the same CLIP RN50 against one prompt per CLASS of the dataset; passes when the softmax over all class prompts gives
    the source image's class at least `1 / n_classes / discount`.  A softmax probability needs the image norm and `logit_scale`
    (an argmax does not), so the row of logits, its softmax and the entries the decisions read are one kernel, `ops.class_head`.

Mirrored text, declared: `NEGATIVE_PROMPTS` and the five `CLASS_PROMPT_TEMPLATES` strings are the reference's wording (:307, :278-295)
because they ARE the contract -- the strings CLIP sees.

MI355X-first choices: BatchNorm (inference) is folded into the conv weights + a bias at pack time, ReLU rides in the GEMM
epilogue (`SASPA_ACT_RELU`, `SASPA_ACT_ADD_RELU` for the bottleneck's add-then-ReLU), pooling is one streaming kernel,
pre-processing (PIL-exact bicubic / bilinear resize, crop, normalise) runs on the device from the decoded u8 image, images
are processed in batches.  Both models run on the exact-fp32 MFMA path by default: the whole stage is ~12 GFLOP per image
(0.01 % of generating it), and an argmax / top-k decision should not move with bf16 rounding.

No CPU or eager-PyTorch arithmetic: torch is used for device memory and layout copies (cat / transpose) only."""
import logging
import os
from pathlib import Path

import numpy as np
import torch

from . import imageproc, models, ops
from . import weights as W
from .config import CLIP_RN50, LPIPS_ALEX, LPIPS_SCALE, LPIPS_SHIFT, WSDAN_CAL_R50, WSDAN_CAL_R101

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
NEGATIVE_PROMPTS = ["a photo of an object", "a photo of a scene", "a photo of geometric shapes", "a photo", "an image",
                    "a black photo"]                                     # all_utils/utils.py:307
# the class prompts of the per-class CLIP filter, per dataset (all_utils/utils.py:277-295); `{name}` = a class / part string
CLASS_PROMPT_TEMPLATES = {
    "planes": "a photo of a {name}, a type of aircraft.",
    "synthetic": "a photo of a {name}, a type of aircraft.",
    "cars": "a photo of a {name}, a type of car.",
    "dtd": "a photo of a {name}, a type of texture.",
    "cub": "a photo of a {name}, a type of a bird.",
    "compcars-parts": "a photo of the {name}, of a car.",
}
RELU, ADD_RELU = ops.ACT_RELU, ops.ACT_ADD_RELU


def _center_crop_origin(length, size):
    return int(round((length - size) / 2.0))        # torchvision.transforms.functional.center_crop (Python round)


def rn50_preprocess(src_u8, dtype, size=224):
    """clip._transform(n_px): Resize(n_px, BICUBIC) of the shorter side, CenterCrop(n_px), /255, CLIP mean / std, on a
    device u8 [n,H,W,3] batch -> [n,size,size,8]."""
    n, h, w, _ = src_u8.shape
    if h <= w:
        oh, ow = size, int(size * w / h)
    else:
        oh, ow = int(size * h / w), size
    top, left = _center_crop_origin(oh, size), _center_crop_origin(ow, size)
    x = imageproc.resize_u8(src_u8.contiguous(), oh, ow, crop=(top, left, size, size), filt="bicubic")
    return imageproc.normalize_u8(x, dtype)


def cal_preprocess(src_u8, dtype, size=224):
    """BaseUtils.get_transform (all_utils/dataset_utils.py:77-85): Resize((size/0.875,)*2) bilinear, CenterCrop(size),
    ToTensor, Normalize(ImageNet)."""
    big = int(size / 0.875)
    o = _center_crop_origin(big, size)
    x = imageproc.resize_u8(src_u8.contiguous(), big, big, crop=(o, o, size, size), filt="bilinear")
    return imageproc.normalize_u8(x, dtype, IMAGENET_MEAN, IMAGENET_STD)


class _Convs:
    """Bias-free convs with their BatchNorm folded in, packed for the implicit-GEMM kernel."""

    def __init__(self, sd, dev, dtype):
        self.sd, self.dev, self.dtype, self.p = sd, dev, dtype, {}

    def conv_bn(self, name, conv, bn, eps=1e-5):
        w, b = W.fold_bn(self.sd[conv + ".weight"], self.sd, bn, eps)
        kh, kw = w.shape[2], w.shape[3]
        pk = W.pack_conv(w)
        chunk = W.chunk_major_ok(kh, kw, W.round8(w.shape[1]), 0, self.dtype)
        if chunk:
            pk = W.to_chunk_major(pk, kh * kw, self.dtype)
        t = pk.to(self.dev, self.dtype)
        t.saspa_korder = 1 if chunk else 0
        self.p[name + ".w"], self.p[name + ".b"], self.p[name + ".k"] = t, b.to(self.dev, torch.float32).contiguous(), (kh, kw)

    def conv_bias(self, name, conv):
        """A conv with its own bias and no BatchNorm (AlexNet)."""
        w = self.sd[conv + ".weight"].float()
        kh, kw = w.shape[2], w.shape[3]
        pk = W.pack_conv(w)
        chunk = W.chunk_major_ok(kh, kw, W.round8(w.shape[1]), 0, self.dtype)
        if chunk:
            pk = W.to_chunk_major(pk, kh * kw, self.dtype)
        t = pk.to(self.dev, self.dtype)
        t.saspa_korder = 1 if chunk else 0
        self.p[name + ".w"], self.p[name + ".k"] = t, (kh, kw)
        self.p[name + ".b"] = self.sd[conv + ".bias"].to(self.dev, torch.float32).contiguous()

    def run(self, name, x, stride=1, pad=0, act=RELU, residual=None):
        kh, kw = self.p[name + ".k"]
        return ops.conv(x, self.p[name + ".w"], self.p[name + ".b"], kh=kh, kw=kw, stride=stride, pad=pad, act=act,
                        residual=residual)


class ClipRN50Visual:
    """clip.model.ModifiedResNet + AttentionPool2d (keys `visual.*` of the OpenAI checkpoint)."""

    def __init__(self, sd, cfg, dev, dtype=torch.float32):
        self.cfg, self.dev, self.dtype = cfg, dev, dtype
        c = self.c = _Convs(sd, dev, dtype)
        v = "visual"
        for i in (1, 2, 3):
            c.conv_bn(f"stem{i}", f"{v}.conv{i}", f"{v}.bn{i}")
        self.blocks = []
        for li, nb in enumerate(cfg["layers"]):
            for bi in range(nb):
                pf = f"{v}.layer{li + 1}.{bi}"
                for j in (1, 2, 3):
                    c.conv_bn(f"{pf}.c{j}", f"{pf}.conv{j}", f"{pf}.bn{j}")
                ds = pf + ".downsample.0.weight" in sd
                if ds:
                    c.conv_bn(f"{pf}.ds", f"{pf}.downsample.0", f"{pf}.downsample.1")
                self.blocks.append((pf, 2 if (bi == 0 and li > 0) else 1, ds))
        a = v + ".attnpool"
        pos = sd[a + ".positional_embedding"].double()
        p = self.p = {}
        for n in ("q", "k", "v"):
            wt, bs = sd[f"{a}.{n}_proj.weight"], sd[f"{a}.{n}_proj.bias"]
            p[n + ".w"] = wt.contiguous().to(dev, dtype)
            # (t + pos) @ W^T + b = t @ W^T + (pos @ W^T + b): the position table becomes a per-token additive term
            p[n + ".r"] = (pos @ wt.double().t() + bs.double()).float().to(dev, dtype).contiguous()
        p["c.w"] = sd[a + ".c_proj.weight"].contiguous().to(dev, dtype)
        p["c.b"] = sd[a + ".c_proj.bias"].float().to(dev).contiguous()
        self.heads = cfg["heads"]
        c.sd = None

    def forward(self, pixels):
        """[B,S,S,8] normalised channels-last pixels -> [B, embed_dim] (dtype of the tower)."""
        c = self.c
        x = c.run("stem1", pixels, stride=2, pad=1)
        x = c.run("stem2", x, pad=1)
        x = c.run("stem3", x, pad=1)
        x = ops.pool2d(x, 2)
        for pf, stride, ds in self.blocks:
            out = c.run(pf + ".c1", x)
            out = c.run(pf + ".c2", out, pad=1)
            if stride > 1:
                out = ops.pool2d(out, stride)
            identity = x
            if ds:
                identity = c.run(pf + ".ds", ops.pool2d(x, stride) if stride > 1 else x, act=ops.ACT_NONE)
            x = c.run(pf + ".c3", out, act=ADD_RELU, residual=identity)
        b, hh, ww, ch = x.shape
        n = hh * ww
        mean = ops.pool2d(x, hh)                                             # the mean token (hh == ww)
        t = torch.cat([mean.view(b, 1, ch), x.view(b, n, ch)], 1).contiguous()   # [B, n+1, C]  (layout copy)
        p = self.p
        nt = n + 1

        def proj(name, rows):
            r = p[name + ".r"][:rows]
            return ops.linear(t[:, :rows].contiguous() if rows != nt else t, p[name + ".w"],
                              residual=r[None].expand(b, -1, -1).contiguous())
        q = proj("q", 1)                                                      # query = the mean token only
        k = proj("k", nt)
        vmat = proj("v", nt)
        ld = ops.round8(nt)
        vt = torch.zeros((b, ch, ld), device=x.device, dtype=x.dtype)
        vt[:, :, :nt] = vmat[:, :, :ch].transpose(1, 2)                       # keys contiguous (layout copy)
        o = models.attention_core(q, k, vt, self.heads, 1, nt)
        return ops.linear(o.view(b, ch), p["c.w"], p["c.b"])


def clip_text_unit_rows(sd, cfg, dev, prompts, tokenizer, dtype=torch.float32, chunk=64):
    """The CLIP text tower over `prompts`, `chunk` prompts per pass -> unit text embeddings fp32 [len(prompts), embed_dim]: a
    constant of the run (TextEncoder + `text_features / text_features.norm()`, all_utils/utils.py:113-134, :161)."""
    tcfg = dict(vocab=cfg["vocab"], width=cfg["text_width"], layers=cfg["text_layers"], heads=cfg["text_heads"],
                mlp=4 * cfg["text_width"], max_pos=cfg["context"])
    text = models.CLIPText(W.openai_clip_text_to_hf(sd, cfg["text_layers"]), tcfg, dev, dtype)
    out = []
    for i in range(0, len(prompts), chunk):
        ids = np.concatenate([tokenizer(pr) for pr in prompts[i:i + chunk]])   # [k, 77]
        ids_t = ops.h2d(torch.from_numpy(ids), dev)
        hidden = text.forward(ids_t)                                          # final-LN states [k, 77, width]
        eot = ids_t.argmax(dim=-1)                                            # clip: the EOT token has the highest id
        rows = hidden[torch.arange(ids.shape[0], device=dev), eot].contiguous()
        feats = ops.linear(rows.float(), text.p["text_projection.w"].float())[:, :cfg["embed_dim"]]
        out.append(torch.nn.functional.normalize(feats.double(), dim=-1).float())
    return (torch.cat(out) if len(out) > 1 else out[0]).contiguous()


class _ClipImageSide:
    """What the two CLIP filters share: the image tower (one `ClipRN50Visual` may serve both) and the embedding of a batch."""

    @torch.no_grad()
    def embed(self, images_u8):
        """device u8 [n,H,W,3] -> fp32 [n, embed_dim] UNNORMALISED image embeddings."""
        px = rn50_preprocess(images_u8, self.dtype, self.cfg["image_size"])
        return self.visual.forward(px)[:, :self.cfg["embed_dim"]].float().contiguous()


class SemanticFilter(_ClipImageSide):
    """CLIP_selector (all_utils/utils.py:137-166) with the prompts [positive] + NEGATIVE_PROMPTS; `passes(images)` is
    `get_semantic_filtering` for a batch: argmax over the prompts == 0.  `visual`: an image tower built elsewhere (the per-class
    filter's) to share."""

    def __init__(self, sd, cfg, dev, positive_prompt, tokenizer, dtype=torch.float32, visual=None):
        self.cfg, self.dev, self.dtype = cfg, dev, dtype
        self.visual = visual if visual is not None else ClipRN50Visual(sd, cfg, dev, dtype)
        self.prompts = [positive_prompt] + NEGATIVE_PROMPTS
        # constant for the run: unit text embeddings (the image norm and logit_scale are common factors of the argmax)
        self.text_unit = clip_text_unit_rows(sd, cfg, dev, self.prompts, tokenizer, dtype)

    @torch.no_grad()
    def logits(self, images_u8, embedding=None):
        """device u8 [n,H,W,3] -> fp32 [n, 7] cosine-similarity logits up to the common positive factor.  `embedding`: the batch's
        `embed()` when the caller already has it."""
        e = self.embed(images_u8) if embedding is None else embedding
        return ops.linear(e, self.text_unit)[:, :len(self.prompts)]

    def passes(self, images_u8, embedding=None):
        return np.argmax(self.logits(images_u8, embedding).cpu().numpy(), axis=-1) == 0       # the decision is host control flow


def class_prompts(ds_utils):
    """(class list, prompts) of the per-class CLIP filter for a dataset (all_utils/utils.py:274-299).  The class list is
    `sorted(set(get_classes()))` -- the reference indexes an unordered set; the decision does not depend on the order -- and
    compcars-parts asks about the photographed PART (`sorted(part_to_string.values())`)."""
    name = getattr(ds_utils, "name", None)
    if name not in CLASS_PROMPT_TEMPLATES:
        raise NotImplementedError(f"per-class CLIP filter: no class prompts for dataset {name!r}")
    if name == "compcars-parts":
        classes = sorted(set(ds_utils.part_to_string.values()))
    else:
        classes = sorted(set(ds_utils.get_classes()))
    return classes, [CLASS_PROMPT_TEMPLATES[name].format(name=c) for c in classes]


def class_labels(ds_utils, original_images_paths, classes):
    """{original file name: index of its class in `classes`} (all_utils/utils.py:384-389): planes / synthetic / cars look the class
    string up by `stem.split("_")[0]` in the stem-keyed dict, the others by image path (compcars-parts: the part folder)."""
    index = {c: i for i, c in enumerate(classes)}
    name = ds_utils.name
    if name in ("planes", "synthetic", "cars"):
        table = ds_utils.get_image_stem_to_class_str_dict()
        return {Path(ip).name: index[table[Path(ip).stem.split("_")[0]]] for ip in original_images_paths}
    if name == "compcars-parts":
        return {Path(ip).name: index[ds_utils.part_to_string[Path(ip).parent.name]] for ip in original_images_paths}
    table = ds_utils.get_image_path_to_class_str_dict()
    return {Path(ip).name: index[table[ip]] for ip in original_images_paths}


def class_threshold(n_classes, discount=1):
    """`threhold = 1 / len(classnames) / clip_filtering_discount` (all_utils/utils.py:303): chance level, divided by the discount."""
    return 1 / n_classes / discount


class ClassFilter(_ClipImageSide):
    """CLIP_selector with one prompt per class (`template.format(name=class)`) and `get_clip_filtering` for a batch
    (all_utils/utils.py:180-191): softmax(logit_scale.exp() * unit(image) @ unit(text)^T)[label] >= 1 / n_classes / discount.
    The unit text matrix [C, embed_dim] and the scale are constants of the run; per batch the image tower runs once and one
    `ops.class_head` launch turns the embeddings into the probabilities."""

    def __init__(self, sd, cfg, dev, class_names, template, tokenizer, discount=1, dtype=torch.float32, visual=None):
        if not class_names:
            raise ValueError("the per-class CLIP filter needs at least one class")
        self.cfg, self.dev, self.dtype = cfg, dev, dtype
        self.visual = visual if visual is not None else ClipRN50Visual(sd, cfg, dev, dtype)
        self.class_names = list(class_names)
        self.prompts = [template.format(name=c) for c in self.class_names]
        self.text_unit = clip_text_unit_rows(sd, cfg, dev, self.prompts, tokenizer, dtype)
        self.scale = float(sd["logit_scale"].float().exp())                   # logit_scale.exp(), a constant of the checkpoint
        self.discount = discount
        self.threshold = class_threshold(len(self.class_names), discount)

    @torch.no_grad()
    def probs(self, images_u8, labels, embedding=None):
        """device u8 [n,H,W,3], labels (host ints, one per image, each in [0, C)) -> fp32 [n] on the device: the softmax probability
        of every image's own class.  Labels are validated HERE (the kernel only marks a bad row with NaN)."""
        lb = np.asarray(labels).astype(np.int64).reshape(-1)
        n = images_u8.shape[0] if embedding is None else embedding.shape[0]
        if lb.size != n or (lb.size and (lb.min() < 0 or lb.max() >= len(self.class_names))):
            raise ValueError(f"labels must hold {n} values in [0, {len(self.class_names)})")
        e = self.embed(images_u8) if embedding is None else embedding
        stats, _, _ = ops.class_head(e, ops.h2d(torch.from_numpy(lb.astype(np.int32)), e.device), self.text_unit, self.scale, True,
                                     width=self.cfg["embed_dim"])
        return stats[:, 1]

    def passes(self, images_u8, labels, embedding=None):
        return self.probs(images_u8, labels, embedding).cpu().numpy().astype(np.float64) >= self.threshold   # host control flow


class WSDANCAL:
    """WSDAN_CAL.forward in eval mode -> p (logits [B, num_classes]); resnet features, 1x1 attention conv + BN + ReLU,
    bilinear attention pooling (GAP form), sign-sqrt, L2 normalise, fc(feature_matrix * 100)."""

    def __init__(self, sd, cfg, dev, dtype=torch.float32):
        self.cfg, self.dev, self.dtype = cfg, dev, dtype
        c = self.c = _Convs(sd, dev, dtype)
        c.conv_bn("stem", "features.0", "features.1")
        self.blocks = []
        strides = (1, 2, 2, 1)      # fgvc ResNet(..., stride=1): layer4 is NOT strided (features at 1/16, 14 x 14 for 224 crops)
        for li, nb in enumerate(cfg["layers"]):
            for bi in range(nb):
                pf = f"features.{4 + li}.{bi}"
                for j in (1, 2, 3):
                    c.conv_bn(f"{pf}.c{j}", f"{pf}.conv{j}", f"{pf}.bn{j}")
                ds = pf + ".downsample.0.weight" in sd
                if ds:
                    c.conv_bn(f"{pf}.ds", f"{pf}.downsample.0", f"{pf}.downsample.1")
                self.blocks.append((pf, strides[li] if bi == 0 else 1, ds))
        wa, ba = W.fold_bn(sd["attentions.conv.weight"], sd, "attentions.bn", 1e-3)        # BasicConv2d: BN eps 0.001
        self.att_w = wa[:, :, 0, 0].contiguous().to(dev, dtype)                           # [M, C]
        self.att_b = ba.to(dev, dtype).contiguous()                                       # per attention map
        self.fc_w = sd["fc.weight"].contiguous().to(dev, torch.float32)
        self.num_classes = self.fc_w.shape[0]
        c.sd = None

    @torch.no_grad()
    def forward(self, pixels):
        c = self.c
        x = c.run("stem", pixels, stride=2, pad=3)
        x = ops.pool2d(x, 3, 2, 1, mode="max")
        for pf, stride, ds in self.blocks:
            out = c.run(pf + ".c1", x)
            out = c.run(pf + ".c2", out, stride=stride, pad=1)
            identity = c.run(pf + ".ds", x, stride=stride, act=ops.ACT_NONE) if ds else x
            x = c.run(pf + ".c3", out, act=ADD_RELU, residual=identity)
        b, hh, ww, ch = x.shape
        hw, m = hh * ww, self.att_w.shape[0]
        ld = ops.round8(hw)
        feat = x.view(b, hw, ch)
        # attention maps TRANSPOSED (swapped GEMM operands, like the V^T projection): att_t[b] = relu(Wa @ feat_b^T + ba)
        att_t = torch.zeros((b, m, ld), device=x.device, dtype=x.dtype)
        bias_t = torch.zeros((b, m, ld), device=x.device, dtype=x.dtype)          # per-row bias as the GEMM's residual
        bias_t[:, :, :hw] = self.att_b[None, :, None]
        ops.gemm_batched(self.att_w, self.att_w.stride(0), (0, 0), feat, feat.stride(1), (feat.stride(0), 0), att_t, ld, (m * ld, 0),
                         m, hw, ch, b, 1, residual=bias_t, ldr=ld, act=ADD_RELU)
        feat_t = torch.zeros((b, ch, ld), device=x.device, dtype=x.dtype)
        feat_t[:, :, :hw] = feat.transpose(1, 2)                                           # layout copy
        # feature_matrix[b] = att_t[b] @ feat_t[b]^T / HW  -> [M, C]
        fm = torch.empty((b, m, ch), device=x.device, dtype=x.dtype)
        ops.gemm_batched(att_t, ld, (m * ld, 0), feat_t, ld, (ch * ld, 0), fm, ch, (m * ch, 0), m, ch, ld, b, 1, alpha=1.0 / hw)
        fm = ops.signsqrt_l2norm(fm.view(b, m * ch).float(), 1e-6, 100.0)
        return ops.linear(fm, self.fc_w)[:, :self.num_classes]


class ConfidenceFilter:
    def __init__(self, sd, cfg, dev, top_k=10, dtype=torch.float32, too_high=None):
        self.cfg, self.dev, self.dtype = cfg, dev, dtype
        self.model = WSDANCAL(sd, cfg, dev, dtype)
        self.top_k = min(int(top_k), self.model.num_classes)                  # all_utils/utils.py:319
        self.too_high = too_high or None                                      # `if filter_confidence_higher_than:` (:368)

    @torch.no_grad()
    def logits(self, images_u8):
        return self.model.forward(cal_preprocess(images_u8, self.dtype, self.cfg["image_size"]))

    def passes(self, images_u8, labels):
        """`correct_label in logits.topk(k)[1]` per image (all_utils/utils.py:363-364); labels: ints, one per image."""
        if self.too_high is None:
            lg = self.logits(images_u8).float().cpu().numpy()                  # the decision is host control flow
            return np.array([int((row > row[int(lb)]).sum()) < self.top_k for lb, row in zip(labels, lg)], dtype=bool)
        return self.passes_and_too_high(images_u8, labels)

    @torch.no_grad()
    def passes_and_too_high(self, images_u8, labels):
        """(top-k mask, too-high mask) from ONE logits-mode `ops.class_head` launch on the classifier's logits: the label is in the
        top k when fewer than k logits are strictly greater, and it is too confident when softmax(logits)[label] > too_high
        (all_utils/utils.py:363-373).  The second mask is False wherever the first is: the reference tests it in the `elif`."""
        lb = np.asarray(labels).astype(np.int64).reshape(-1)
        if lb.size != images_u8.shape[0] or (lb.size and (lb.min() < 0 or lb.max() >= self.model.num_classes)):
            raise ValueError(f"labels must hold {images_u8.shape[0]} values in [0, {self.model.num_classes})")
        lg = self.logits(images_u8).float()
        stats, idx, _ = ops.class_head(lg, ops.h2d(torch.from_numpy(lb.astype(np.int32)), lg.device), width=self.model.num_classes)
        in_top_k = idx[:, 1].cpu().numpy() < self.top_k                         # the decisions are host control flow
        high = stats[:, 1].cpu().numpy().astype(np.float64) > (self.too_high if self.too_high is not None else np.inf)
        return in_top_k, high & in_top_k


class LpipsAlex:
    """`lpips.LPIPS(net='alex')` (v0.1) for batches of pairs: ScalingLayer, torchvision AlexNet `features` up to each of the five ReLUs,
    and per level unit-normalise / difference / square / `lin` weights / spatial mean in ONE kernel (ops.lpips_layer); the five levels
    sum into one fp32 vector.  The originals' features are computed once and shared by their augmentations through `ref_index`."""
    STRIDE_PAD = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))

    def __init__(self, sd, cfg, dev, dtype=torch.float32):
        self.cfg, self.dev, self.dtype = cfg, dev, dtype
        c = self.c = _Convs(sd, dev, dtype)
        for i, (idx, _) in enumerate(W.LPIPS_ALEX_CONVS):
            c.conv_bias(f"c{i}", f"features.{idx}")
        self.lin = []
        for i, ch in enumerate(cfg["channels"]):
            w = sd[f"lin{i}.model.1.weight"].reshape(-1).float()
            if w.numel() != ch or bool((w < 0).any()):
                raise ValueError(f"lin{i}: expected {ch} non-negative channel weights")
            self.lin.append(w.contiguous().to(dev))
        # [0, 1] -> [-1, 1] -> ScalingLayer, folded: (2x - 1 - shift) / scale = (x - (1 + shift) / 2) / (scale / 2)
        self.mean = tuple((1.0 + sh) / 2.0 for sh in LPIPS_SHIFT)
        self.std = tuple(sc / 2.0 for sc in LPIPS_SCALE)
        c.sd = None

    def preprocess(self, images_u8, resize=(256, 256), grey=True):
        """device u8 [k,H,W,3] -> [k,h,w,8] network input: `convert("L").convert("RGB")` (grey), `Image.resize(resize)` (PIL's
        default filter, BICUBIC; `resize` = (width, height) like PIL), ToTensor, x * 2 - 1, ScalingLayer."""
        x = images_u8.contiguous()
        if grey:
            x = ops.u8_luma(x)
        if resize:
            x = imageproc.resize_u8(x, int(resize[1]), int(resize[0]), filt="bicubic")
        return imageproc.normalize_u8(x, self.dtype, self.mean, self.std)

    def features(self, pixels):
        """The five ReLU outputs, channels-last as ops.conv leaves them."""
        c, feats, x = self.c, [], pixels
        for i, (stride, pad) in enumerate(self.STRIDE_PAD):
            if i in (1, 2):
                x = ops.pool2d(x, 3, 2, 0, mode="max")
            x = c.run(f"c{i}", x, stride=stride, pad=pad)
            feats.append(x)
        return feats

    @torch.no_grad()
    def distance(self, aug_px, ref_px, ref_index):
        """Pre-processed batches [n,h,w,8] / [m,h,w,8] (same h, w) and ref_index (host ints or a tensor, one per augmentation)
        -> fp32 [n] on the device.  ref_index is validated HERE (the kernel trusts it)."""
        n, m = aug_px.shape[0], ref_px.shape[0]
        if tuple(aug_px.shape[1:]) != tuple(ref_px.shape[1:]):
            raise ValueError(f"LPIPS needs both images of a pair at one size, got {tuple(aug_px.shape[1:3])} and {tuple(ref_px.shape[1:3])}")
        idx = np.asarray(ref_index.cpu() if torch.is_tensor(ref_index) else ref_index).astype(np.int64).reshape(-1)
        if idx.size != n or (idx.size and (idx.min() < 0 or idx.max() >= m)):
            raise ValueError(f"ref_index must hold {n} values in [0, {m})")
        idx_d = ops.h2d(torch.from_numpy(idx.astype(np.int32)), aug_px.device)
        fa, fr = self.features(aug_px), self.features(ref_px)
        dist = torch.empty((n,), device=aug_px.device, dtype=torch.float32)
        ws = torch.empty((n * ops._lib.LPIPS_MAX_BLOCKS,), device=aug_px.device, dtype=torch.float32)
        for i, (a, r) in enumerate(zip(fa, fr)):
            ch = self.cfg["channels"][i]
            ops.lpips_layer(a[..., :ch] if a.shape[-1] != ch else a, r[..., :ch] if r.shape[-1] != ch else r, idx_d, self.lin[i],
                            dist, accumulate=i > 0, workspace=ws)
        return dist

    def forward(self, aug_u8, ref_u8, ref_index, resize=(256, 256), grey=True):
        """Two device u8 batches [n,H,W,3] / [m,H',W',3] -> fp32 [n]: d(ref_u8[ref_index[j]], aug_u8[j]).  `resize=None` keeps the
        sizes; a pair of unequal sizes is then a ValueError (the reference would fail inside the network)."""
        if not resize and tuple(aug_u8.shape[1:3]) != tuple(ref_u8.shape[1:3]):
            raise ValueError(f"LPIPS without resize needs equal sizes, got {tuple(aug_u8.shape[1:3])} and {tuple(ref_u8.shape[1:3])}")
        return self.distance(self.preprocess(aug_u8, resize, grey), self.preprocess(ref_u8, resize, grey), ref_index)


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def load_cal_checkpoint(path):
    """A baseline-classifier checkpoint as fgvc/train.py saves it ({'state_dict': ...}; keys possibly prefixed with
    `_orig_mod.` by torch.compile, all_utils/dataset_utils.py:99-104) -> (state dict, config)."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck["state_dict"] if "state_dict" in ck else ck
    sd = {k.replace("_orig_mod.", "").replace("module.", ""): v.float() for k, v in sd.items()
          if torch.is_tensor(v) and not k.endswith("num_batches_tracked")}
    n23 = any(k.startswith("features.6.22.") for k in sd)
    cfg = dict(WSDAN_CAL_R101 if n23 else WSDAN_CAL_R50, num_classes=sd["fc.weight"].shape[0])
    return sd, cfg


def load_clip_rn50(path):
    """OpenAI's RN50.pt (a TorchScript archive) or a plain state-dict file -> fp32 state dict."""
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    return {k: v.float() for k, v in sd.items() if torch.is_tensor(v)}


def synthetic_filters_allowed():
    """Opt-in for architecture-exact SYNTHETIC filter weights (tests, benchmarks): SASPA_SYNTHETIC_FILTERS=1."""
    return os.environ.get("SASPA_SYNTHETIC_FILTERS", "0") not in ("", "0")


def filter_checkpoints(ds_utils, weights_dir, semantic=True, confidence=True, per_class=False):
    """Paths of the checkpoints the enabled filters need: (clip RN50 path | None, baseline checkpoint path | None); the per-class
    CLIP filter (`per_class`) reads the same `clip/RN50.pt` as the semantic filter.
    Raises FileNotFoundError for a missing / ambiguous checkpoint unless synthetic filter weights were asked for
    explicitly -- a filtered aug.json must never reflect the decisions of random models (the reference asserts exactly
    one baseline checkpoint, all_utils/dataset_utils.py:92, and loads the real CLIP, all_utils/utils.py:253)."""
    name = "compcars" if "compcars" in ds_utils.name else ds_utils.name
    rn = cp = None
    if semantic or per_class:
        cand = os.path.join(weights_dir, "clip", "RN50.pt") if weights_dir else None
        if cand and os.path.exists(cand):
            rn = cand
        elif not synthetic_filters_allowed():
            which, knob = ("semantic filter", "SEMANTIC_FILTERING = 0") if semantic else ("per-class CLIP filter", "CLIP_FILTERING_TYPE = None")
            raise FileNotFoundError(
                f"{which}: {cand or '<WEIGHTS_DIR>/clip/RN50.pt'} not found.  Give WEIGHTS_DIR with the OpenAI CLIP RN50 "
                f"checkpoint, set {knob}, or opt in to synthetic filter weights with SASPA_SYNTHETIC_FILTERS=1")
    if confidence:
        cdir = Path(weights_dir, "checkpoints", name) if weights_dir else None
        cps = sorted(cdir.glob("*.pth")) if cdir else []
        if len(cps) > 1:
            raise FileNotFoundError(f"Found {len(cps)} checkpoints in {cdir}. Expected 1")
        if cps:
            cp = str(cps[0])
        elif not synthetic_filters_allowed():
            raise FileNotFoundError(
                f"model-confidence filter: no baseline checkpoint (*.pth) in {cdir or '<WEIGHTS_DIR>/checkpoints/' + name}.  Train the "
                "baseline first (fgvc/train.py), set MODEL_CONFIDENCE_BASED_FILTERING = 0, or opt in to synthetic filter "
                "weights with SASPA_SYNTHETIC_FILTERS=1")
    return rn, cp


def lpips_checkpoints(weights_dir):
    """(torchvision AlexNet file, lpips `alex.pth`) under `<weights_dir>/lpips/` -- `alexnet*.pth` (torchvision ships it as
    alexnet-owt-7be5be79.pth) and `alex.pth` -- or (None, None) when synthetic filter weights were asked for.  The rule of
    `filter_checkpoints`: a missing file is a FileNotFoundError unless SASPA_SYNTHETIC_FILTERS=1."""
    d = Path(weights_dir, "lpips") if weights_dir else None
    nets = sorted(p for p in d.glob("alexnet*.pth")) if d else []
    lin = d / "alex.pth" if d else None
    if len(nets) == 1 and lin.exists():
        return str(nets[0]), str(lin)
    if len(nets) > 1:
        raise FileNotFoundError(f"Found {len(nets)} alexnet*.pth files in {d}. Expected 1")
    if synthetic_filters_allowed():
        return None, None
    raise FileNotFoundError(
        f"LPIPS filter: {d or '<WEIGHTS_DIR>/lpips'} must hold torchvision's AlexNet weights (alexnet*.pth) and the lpips package's "
        "alex.pth.  Give WEIGHTS_DIR, set LPIPS_MIN = LPIPS_MAX = None, or opt in to synthetic filter weights with "
        "SASPA_SYNTHETIC_FILTERS=1")


N_PARAMS_ALEX_FEATURES, N_PARAMS_LPIPS_LIN = 2469696, 1152


def load_lpips_alex(alex_path, lin_path):
    """The two checkpoints -> one fp32 state dict with the keys `weights.lpips_alex_spec` names (the classifier half of the
    torchvision file is dropped; a `net.`/`module.` prefix is tolerated)."""
    sd = {}
    for path, keep in ((alex_path, "features."), (lin_path, "lin")):
        ck = torch.load(path, map_location="cpu", weights_only=True)
        ck = ck["state_dict"] if "state_dict" in ck else ck
        for k, v in ck.items():
            k = k.replace("module.", "")
            if torch.is_tensor(v) and k.startswith(keep):
                sd[k] = v.float()
    want = {n: tuple(shape) for n, shape, _ in W.lpips_alex_spec(LPIPS_ALEX)}
    bad = [n for n, shape in want.items() if n not in sd or tuple(sd[n].shape) != shape]
    if bad:
        raise KeyError(f"LPIPS checkpoints {alex_path}, {lin_path}: missing / mis-shaped tensors {bad[:4]}")
    sd = {n: sd[n] for n in want}
    nf = sum(v.numel() for k, v in sd.items() if k.startswith("features."))
    assert (nf, sum(v.numel() for v in sd.values()) - nf) == (N_PARAMS_ALEX_FEATURES, N_PARAMS_LPIPS_LIN)
    return sd


def build_lpips(dev, weights_dir=None):
    """The LPIPS model of the lpips_min / lpips_max filter and the diversity measure; checkpoints by `lpips_checkpoints`."""
    net, lin = lpips_checkpoints(weights_dir)
    if net:
        sd = load_lpips_alex(net, lin)
    else:
        logging.warning("LPIPS filter: SASPA_SYNTHETIC_FILTERS=1 -> SYNTHETIC AlexNet / lin weights; its distances are those of a random model")
        sd = W.synth_state_dict("lpips_alex", LPIPS_ALEX, 13)
    return LpipsAlex(sd, LPIPS_ALEX, dev)


def build_filters(ds_utils, dev, semantic=True, confidence=True, weights_dir=None, top_k=10, tokenizer=None, per_class=False,
                  discount=1, too_high=None):
    """The filter models for a dataset: (semantic, confidence), and with `per_class` (semantic, confidence, per-class CLIP filter).
    `weights_dir` holds `clip/RN50.pt` and `checkpoints/<dataset>/*.pth` (the reference's `all_utils/checkpoints/<name>/`).  A
    missing checkpoint is an error (filter_checkpoints); only with SASPA_SYNTHETIC_FILTERS=1 does the stage run on
    architecture-exact SYNTHETIC weights, and says so loudly.  The two CLIP filters share one image tower (the reference loads one
    `clip.load('RN50')` for both, all_utils/utils.py:252-255)."""
    from .tokenizer import make_tokenizer
    sem = conf = cls = None
    rn, cp = filter_checkpoints(ds_utils, weights_dir, semantic, confidence, per_class)
    if semantic or per_class:
        if rn:
            sd = load_clip_rn50(rn)
        else:
            logging.warning(f"{'semantic' if semantic else 'per-class CLIP'} filter: SASPA_SYNTHETIC_FILTERS=1 -> SYNTHETIC CLIP-RN50 weights; its decisions are those of a random model")
            sd = W.synth_state_dict("clip_rn50", CLIP_RN50, 11)
        tok = tokenizer or make_tokenizer(os.path.join(weights_dir, "clip") if weights_dir else None, CLIP_RN50["vocab"], pad_id=0)
        visual = None
        if per_class:
            classes, _ = class_prompts(ds_utils)
            cls = ClassFilter(sd, CLIP_RN50, dev, classes, CLASS_PROMPT_TEMPLATES[ds_utils.name], tok, discount)
            visual = cls.visual
        if semantic:
            sem = SemanticFilter(sd, CLIP_RN50, dev, ds_utils.get_basic_prompt(), tok, visual=visual)
    if confidence:
        if cp:
            sd, cfg = load_cal_checkpoint(cp)
        else:
            logging.warning("confidence filter: SASPA_SYNTHETIC_FILTERS=1 -> SYNTHETIC WSDAN_CAL (resnet101) weights; its decisions are those of a random model")
            cfg = dict(WSDAN_CAL_R101, num_classes=max(2, ds_utils.num_classes))
            sd = W.synth_state_dict("cal", cfg, 12)
        conf = ConfidenceFilter(sd, cfg, dev, top_k, too_high=too_high)
    return (sem, conf, cls) if per_class else (sem, conf)


# ---------------------------------------------------------------------------------------------------------------------
# the stage itself (all_utils/utils.py:337-437, the filter part of the per-image loop)
# ---------------------------------------------------------------------------------------------------------------------
def _load_u8(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:      # header only: nothing is decoded
        return im.size[1], im.size[0]


def _load_original_u8(path):
    """An original for the LPIPS filter as u8 RGB.  The reference calls `convert("L")` on whatever mode the file decodes to; here
    everything that is not RGB or L (RGBA, CMYK, P ...) goes through `convert("RGB")` first and the device computes the luma."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def lpips_bounds(lpips_min, lpips_max):
    """The reference applies `lpips_min <= d <= lpips_max` when `lpips_min or lpips_max` (all_utils/utils.py:377-379) and dies with a
    TypeError inside its loop when only one is given; here that is a ValueError before anything is read.  -> enabled?"""
    if not (lpips_min or lpips_max):
        return False
    if lpips_min is None or lpips_max is None:
        raise ValueError(f"the LPIPS filter needs both bounds (lpips_min = {lpips_min}, lpips_max = {lpips_max})")
    return True


def _refs_on_device(model, refs, dev, resize, grey, want_hw=None):
    """Pre-process host originals (mixed sizes) one size group at a time -> [m,h,w,8] in the order given."""
    if not resize:
        for r in refs:
            if want_hw is not None and tuple(r.shape[:2]) != tuple(want_hw):
                raise ValueError(f"LPIPS without resize needs equal sizes, got {tuple(r.shape[:2])} and {tuple(want_hw)}")
    out = [None] * len(refs)
    by_size = {}
    for i, r in enumerate(refs):
        by_size.setdefault(r.shape[:2], []).append(i)
    for _, ids in sorted(by_size.items()):
        px = model.preprocess(ops.h2d(torch.from_numpy(np.stack([refs[i] for i in ids])), dev), resize, grey)
        for k, i in enumerate(ids):
            out[i] = px[k:k + 1]
    return torch.cat(out).contiguous() if len(out) > 1 else out[0]


def lpips_pair_distances(model, pairs, dev=None, resize=(256, 256), grey=True, batch_size=32):
    """[(original path, augmented path)] -> [float] LPIPS distances, batched by augmented-image size; an original is decoded once
    per run of consecutive pairs that share it."""
    dev = model.dev if dev is None else dev
    groups = {}
    for k, (op, ap) in enumerate(pairs):
        groups.setdefault(_image_size(ap), []).append(k)
    out = [0.0] * len(pairs)
    for size, ks in sorted(groups.items()):
        for i in range(0, len(ks), batch_size):
            chunk = ks[i:i + batch_size]
            refs, idx, last = [], [], None
            for k in chunk:
                if pairs[k][0] != last:
                    last = pairs[k][0]
                    refs.append(_load_original_u8(last))
                idx.append(len(refs) - 1)
            aug = ops.h2d(torch.from_numpy(np.stack([_load_original_u8(pairs[k][1]) for k in chunk])), dev)
            d = model.distance(model.preprocess(aug, resize, grey), _refs_on_device(model, refs, dev, resize, grey, size), idx)
            for k, v in zip(chunk, d.cpu().tolist()):
                out[k] = v
    return out


def apply_filters(mapping, original_images_paths, ds_utils, dev, semantic=None, confidence=None, batch_size=32, lpips=None,
                  lpips_min=None, lpips_max=None, resize=(256, 256), class_filter=None):
    """mapping: {original file name: [augmented paths]} as `match_augmented_images` builds it (every original present).
    Returns (filtered mapping, counters).  Per original image the reference first drops the augmentations whose
    classifier top-k misses the source label, then those CLIP does not recognise as the meta class; both decisions are
    per augmented image and independent, so they are evaluated in batches (grouped by image size) and combined.
    Memory: a first pass reads only the PNG headers to group the paths by size; pixels are decoded per batch on a
    prefetch thread, so at most two batches are resident on the host (a real dataset has 13-16k augmentations of ~1 MB).
    `lpips` (an LpipsAlex) with both bounds adds the reference's second filter, between the two (:377-381): the augmented batch
    already on the device is reused, every original is decoded once per run of consecutive augmentations of a batch, and a dropped
    image is counted once, under the first filter that drops it (top-k, then LPIPS, then semantic).
    `class_filter` (a ClassFilter) adds the per-class CLIP filter of the Real-Guidance baseline between LPIPS and semantic
    (:383-399; counter `clip_filtering`); when it and the semantic filter share their image tower, the tower runs once per batch.
    A ConfidenceFilter with `too_high` also drops, among the images that pass top-k, those it is too sure of (:368-375; counter
    `too_high_confidence`).  Order of attribution: top-k / too-high, LPIPS, per-class CLIP, semantic."""
    from concurrent.futures import ThreadPoolExecutor
    if dev is None:
        for m in (semantic, confidence, lpips, class_filter):
            if m is not None:
                dev = m.dev
                break
    labels = {}
    if confidence is not None:
        table = ds_utils.get_image_path_to_class_id_dict()
        for ip in original_images_paths:
            labels[Path(ip).name] = table[ip]
    work = [(name, ap) for name, aps in mapping.items() for ap in aps]
    keep = {}
    counters = dict(not_in_top_k=0, semantic=0)
    use_high = confidence is not None and getattr(confidence, "too_high", None) is not None
    if use_high:
        counters["too_high_confidence"] = 0
    if class_filter is not None:
        counters["clip_filtering"] = 0
        cls_labels = class_labels(ds_utils, original_images_paths, class_filter.class_names)
    shared_tower = class_filter is not None and semantic is not None and getattr(semantic, "visual", None) is class_filter.visual
    use_lpips = lpips is not None and lpips_bounds(lpips_min, lpips_max)
    if use_lpips:
        counters["lpips"] = 0
        orig_path = {Path(ip).name: ip for ip in original_images_paths}
    groups = {}
    for name, ap in work:
        groups.setdefault(_image_size(ap), []).append((name, ap))
    chunks = [items[i:i + batch_size] for _, items in sorted(groups.items()) for i in range(0, len(items), batch_size)]

    def decode(chunk):
        pixels = np.stack([_load_u8(ap) for _, ap in chunk])
        refs, idx, last = [], [], None
        if use_lpips:
            for name, _ in chunk:
                if name != last:
                    last = name
                    refs.append(_load_original_u8(orig_path[name]))
                idx.append(len(refs) - 1)
        return pixels, refs, idx

    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(decode, chunks[0]) if chunks else None
        for ci, chunk in enumerate(chunks):
            pixels, refs, idx = nxt.result()
            nxt = pool.submit(decode, chunks[ci + 1]) if ci + 1 < len(chunks) else None
            batch = ops.h2d(torch.from_numpy(pixels), dev)
            ok_c, high = np.ones(len(chunk), bool), np.zeros(len(chunk), bool)
            if use_high:
                ok_c, high = confidence.passes(batch, [labels[name] for name, _ in chunk])
            elif confidence is not None:
                ok_c = confidence.passes(batch, [labels[name] for name, _ in chunk])
            emb = class_filter.embed(batch) if shared_tower else None            # one image-tower pass for both CLIP filters
            ok_p = class_filter.passes(batch, [cls_labels[name] for name, _ in chunk], embedding=emb) if class_filter is not None else np.ones(len(chunk), bool)
            if semantic is None:
                ok_s = np.ones(len(chunk), bool)
            else:
                ok_s = semantic.passes(batch, embedding=emb) if shared_tower else semantic.passes(batch)
            ok_l = np.ones(len(chunk), bool)
            if use_lpips:
                ref_px = _refs_on_device(lpips, refs, dev, resize, True, pixels.shape[1:3])
                d = lpips.distance(lpips.preprocess(batch, resize, True), ref_px, idx).cpu().numpy().astype(np.float64)   # host control flow
                ok_l = (lpips_min <= d) & (d <= lpips_max)
            for (name, ap), c_ok, h_bad, l_ok, p_ok, s_ok in zip(chunk, ok_c, high, ok_l, ok_p, ok_s):
                if not c_ok:
                    counters["not_in_top_k"] += 1          # dropped first: never reaches the other filters (:357-366)
                elif h_bad:
                    counters["too_high_confidence"] += 1   # the `elif` of the same loop (:368-375)
                elif not l_ok:
                    counters["lpips"] += 1                 # second (:377-381)
                elif not p_ok:
                    counters["clip_filtering"] += 1        # third (:383-399)
                elif not s_ok:
                    counters["semantic"] += 1
                keep[ap] = bool(c_ok and not h_bad and l_ok and p_ok and s_ok)
    out = {name: [ap for ap in aps if keep[ap]] for name, aps in mapping.items()}
    return out, counters


# ---------------------------------------------------------------------------------------------------------------------
# the in-line form of the stage (Settings.FILTER_INLINE): threshold-free scores recorded while generating, decisions on the host
# ---------------------------------------------------------------------------------------------------------------------
RECORD_FIELDS = ("valid", "sem_argmax", "sem_margin", "conf_n_greater", "conf_p_label", "pc_p_label", "pc_n_greater", "reserved")
VALID_SEMANTIC, VALID_CONFIDENCE, VALID_PER_CLASS = 1, 2, 4
SCORES_FILE = "filter_scores.json"
SCORES_VERSION = 1


def decide(records, *, semantic, top_k, too_high, pc_threshold):
    """The decisions of `apply_filters` from score records, on the host, without a GPU.  records: fp32 [n, 8] (the fields of
    `saspa_filter_record`).  semantic: apply the semantic filter; top_k: the classifier's k, None = the confidence filter is off;
    too_high: its upper bound on softmax(label) or None; pc_threshold: the per-class CLIP filter's threshold, None = off.
    -> (keep mask bool [n], counters) with the comparisons and the order of attribution of `apply_filters`: top-k
    (`conf_n_greater < top_k`), too-high (`float64(conf_p_label) > too_high`, only where top-k passed), per-class
    (`float64(pc_p_label) >= pc_threshold`), semantic (`sem_argmax == 0`); a dropped image counts once, under the first that drops it.
    A record that lacks a score an enabled filter needs (its `valid` bit is clear, or the row is still NaN) is a ValueError."""
    rec = np.asarray(records, dtype=np.float32).reshape(-1, len(RECORD_FIELDS))
    n = rec.shape[0]
    too_high = too_high or None                                  # `if filter_confidence_higher_than:` (ConfidenceFilter)
    need = (VALID_SEMANTIC if semantic else 0) | (VALID_CONFIDENCE if top_k is not None else 0) | (VALID_PER_CLASS if pc_threshold is not None else 0)
    valid = np.where(np.isnan(rec[:, 0]), 0, rec[:, 0]).astype(np.int64)
    lacking = np.nonzero((valid & need) != need)[0]
    if lacking.size:
        raise ValueError(f"{lacking.size} of {n} records lack a score the enabled filters need (first: row {int(lacking[0])}, valid = {int(valid[lacking[0]])}, needed {need})")
    ok_c, high = np.ones(n, bool), np.zeros(n, bool)
    counters = dict(not_in_top_k=0, semantic=0)
    if top_k is not None:
        ok_c = rec[:, 3] < top_k
        if too_high is not None:
            counters["too_high_confidence"] = 0
            high = (rec[:, 4].astype(np.float64) > too_high) & ok_c
    ok_p = np.ones(n, bool)
    if pc_threshold is not None:
        counters["clip_filtering"] = 0
        ok_p = rec[:, 5].astype(np.float64) >= pc_threshold
    ok_s = rec[:, 1] == 0 if semantic else np.ones(n, bool)
    counters["not_in_top_k"] = int((~ok_c).sum())
    if "too_high_confidence" in counters:
        counters["too_high_confidence"] = int(high.sum())
    alive = ok_c & ~high
    if "clip_filtering" in counters:
        counters["clip_filtering"] = int((alive & ~ok_p).sum())
    alive &= ok_p
    counters["semantic"] = int((alive & ~ok_s).sum())
    return alive & ok_s, counters


class FilterRecorder:
    """The filter models over device-resident batches, scores kept on the device: `record` launches the towers, the heads and
    `ops.filter_record` on the current stream and returns without synchronising; `table_host()` is the one synchronising read, after
    the loop.  Owns the table fp32 [n_rows, 8], NaN = "no record".  The same object scores the batches of the generation loop and the
    PNGs of the backfill, so there is ONE scoring path.  The models keep their dtype: the scores are those of the post-hoc stage."""

    def __init__(self, semantic, confidence, class_filter, n_rows, dev):
        if semantic is None and confidence is None and class_filter is None:
            raise ValueError("FilterRecorder needs at least one filter model")
        self.semantic, self.confidence, self.class_filter, self.dev = semantic, confidence, class_filter, dev
        self.shared_tower = class_filter is not None and semantic is not None and getattr(semantic, "visual", None) is class_filter.visual
        self.n_rows = int(n_rows)
        self.table = torch.full((self.n_rows, len(RECORD_FIELDS)), float("nan"), device=dev, dtype=torch.float32)

    def reset(self, n_rows):
        self.n_rows = int(n_rows)
        self.table = torch.full((self.n_rows, len(RECORD_FIELDS)), float("nan"), device=self.dev, dtype=torch.float32)

    @staticmethod
    def _labels(labels, n, n_classes, what):
        lb = np.asarray(labels).astype(np.int64).reshape(-1)
        if lb.size != n or (lb.size and (lb.min() < 0 or lb.max() >= n_classes)):
            raise ValueError(f"{what} labels must hold {n} values in [0, {n_classes})")
        return lb.astype(np.int32)

    @torch.no_grad()
    def record(self, images_u8, conf_labels, pc_labels, slots, bad=None):
        """device u8 [n,H,W,3]; conf_labels / pc_labels: host ints per image (ignored where that filter is off); slots: host ints, the
        table rows; bad: device bool [n] of images to invalidate, or None.  Everything is validated before the first launch."""
        n = images_u8.shape[0]
        conf, cls, sem = self.confidence, self.class_filter, self.semantic
        cl = self._labels(conf_labels, n, conf.model.num_classes, "classifier") if conf is not None else None
        pl = self._labels(pc_labels, n, len(cls.class_names), "per-class") if cls is not None else None
        c_pair = p_pair = s_logits = None
        if conf is not None:
            lg = conf.logits(images_u8).float()
            stats, idx, _ = ops.class_head(lg, ops.h2d(torch.from_numpy(cl), lg.device), width=conf.model.num_classes)
            c_pair = (stats, idx)
        emb = cls.embed(images_u8) if self.shared_tower else None               # one image-tower pass for both CLIP filters
        if cls is not None:
            e = cls.embed(images_u8) if emb is None else emb
            stats, idx, _ = ops.class_head(e, ops.h2d(torch.from_numpy(pl), e.device), cls.text_unit, cls.scale, True, width=cls.cfg["embed_dim"])
            p_pair = (stats, idx)
        if sem is not None:
            s_logits = sem.logits(images_u8, embedding=emb) if self.shared_tower else sem.logits(images_u8)
        ops.filter_record(self.table, slots, s_logits, c_pair, p_pair, bad)

    def table_host(self):
        return self.table.cpu().numpy()


def recorder_header(semantic, confidence, class_filter, clip_source, cal_source):
    """What the scores of a FilterRecorder depend on, as a JSON-able dict: where the weights came from (a checkpoint path, "synthetic",
    or "handed in" for models the caller built), the prompts of the two CLIP filters (the positive prompt first; the class list through
    its prompts), the classifier's class count, the dtypes.  Two runs may share records only when their headers are equal."""
    h = dict(version=SCORES_VERSION, fields=list(RECORD_FIELDS))
    if semantic is not None:
        h["semantic"] = dict(weights=clip_source, prompts=list(semantic.prompts), dtype=str(semantic.dtype), image_size=semantic.cfg["image_size"])
    if confidence is not None:
        h["confidence"] = dict(weights=cal_source, num_classes=int(confidence.model.num_classes), dtype=str(confidence.dtype),
                               image_size=confidence.cfg["image_size"])
    if class_filter is not None:
        h["per_class"] = dict(weights=clip_source, classes=list(class_filter.class_names), prompts=list(class_filter.prompts),
                              scale=float(np.float32(class_filter.scale)), dtype=str(class_filter.dtype), image_size=class_filter.cfg["image_size"])
    return h


def scores_path(images_folder):
    """`filter_scores.json` beside the aug JSONs: in the parent of `images/`."""
    return str(Path(images_folder).parent / SCORES_FILE)


def _enc(x):
    x = np.float32(x)
    if np.isnan(x):
        return None
    if np.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"              # (JSON has no literal for them; `sem_margin` of a one-prompt filter)
    return float(x)                                               # fp32 -> double is exact and repr(double) round-trips


def _dec(v):
    return np.float32("nan") if v is None else np.float32(v)


def save_scores(path, header, records, sizes):
    """records: {png file name: 8 fp32}; sizes: {png file name: bytes of the PNG the record was taken from}."""
    import json
    body = dict(header=header, records={k: [_enc(x) for x in np.asarray(v, np.float32).reshape(-1)] for k, v in records.items()},
                sizes={k: int(sizes[k]) for k in records})
    tmp = str(path) + ".tmp"
    with open(tmp, "w") as f:
        json.dump(body, f, allow_nan=False)
    os.replace(tmp, path)


def load_scores(path):
    """-> (header, {name: fp32 [8]}, {name: bytes}), or (None, {}, {}) when there is no sidecar."""
    import json
    if not os.path.exists(path):
        return None, {}, {}
    with open(path, "r") as f:
        body = json.load(f)
    recs = {k: np.array([_dec(x) for x in v], np.float32) for k, v in body.get("records", {}).items()}
    return body.get("header"), recs, {k: int(v) for k, v in body.get("sizes", {}).items()}


def merge_scores(images_folder, header, new_records):
    """The sidecar of `images_folder` brought up to date and written: an existing one with an equal header is merged (new records replace
    old ones), a different header discards the old records with a log line; a record whose PNG is gone or whose byte size differs is
    dropped.  -> (records, sizes) as written."""
    path = scores_path(images_folder)
    old_header, records, sizes = load_scores(path)
    if old_header is not None and old_header != header:
        logging.info(f"{path}: written for other filter models / prompts (header differs) -- its {len(records)} records are discarded")
        records, sizes = {}, {}
    for name, rec in new_records.items():
        records[name] = np.asarray(rec, np.float32).reshape(-1)
        sizes.pop(name, None)
    kept, kept_sizes = {}, {}
    for name, rec in records.items():
        try:
            size = os.path.getsize(os.path.join(images_folder, name))
        except OSError:
            continue                                              # the PNG is gone
        if name in sizes and sizes[name] != size:
            continue                                              # another file now carries the name
        kept[name], kept_sizes[name] = rec, size
    if len(kept) != len(records):
        logging.info(f"{path}: dropped {len(records) - len(kept)} stale records (PNG missing or of another size)")
    save_scores(path, header, kept, kept_sizes)
    return kept, kept_sizes


def backfill_scores(recorder, missing, conf_label_of, pc_label_of, planned_batches=None, batch_size=32):
    """Scores for PNGs that have no record -- files an earlier run wrote -- through the SAME `FilterRecorder.record` as the generation
    loop, from decoded pixels.  missing: [png path]; `conf_label_of` / `pc_label_of`: path -> label (or None when the filter is off);
    planned_batches: [[png path]] = the batches the generation loop would have formed: a missing image is scored with the missing images
    of its planned batch, in that order; the rest is grouped by size into chunks of `batch_size`.  -> {png file name: fp32 [8]}."""
    want = list(dict.fromkeys(missing))
    left = set(want)
    chunks = []
    for b in planned_batches or ():
        c = [p for p in b if p in left]
        if c:
            chunks.append(c)
            left -= set(c)
    groups = {}
    for p in want:
        if p in left:
            groups.setdefault(_image_size(p), []).append(p)
    chunks += [items[i:i + batch_size] for _, items in sorted(groups.items()) for i in range(0, len(items), batch_size)]
    order = [p for c in chunks for p in c]
    if not order:
        return {}
    recorder.reset(len(order))
    row = 0
    for c in chunks:
        batch = ops.h2d(torch.from_numpy(np.stack([_load_u8(p) for p in c])), recorder.dev)
        recorder.record(batch, [conf_label_of(p) for p in c] if conf_label_of else None, [pc_label_of(p) for p in c] if pc_label_of else None,
                        list(range(row, row + len(c))))
        row += len(c)
    table = recorder.table_host()
    return {Path(p).name: table[k].copy() for k, p in enumerate(order)}
