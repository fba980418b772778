"""Weights: diffusers-named state dicts (synthetic or from safetensors) and their packing
into the device layout the kernels consume.

The reference loads HF checkpoints (`from_pretrained`, run_aug/run_aug.py:185, :206); there
is no network / no checkpoint in the build and bench environments, so `synth_*` builds
architecture-exact tensors under the SAME key names (a real `*.safetensors` loads through
`load_safetensors` unchanged).  Init: N(0, 1/sqrt(fan_in)) for conv/linear weights, small
biases, norm gains around 1 -- keeps activations O(1) through 50 steps and avoids
all-zero MFMA operands."""
import math
import re

import torch


# --------------------------------------------------------------------------------------
# parameter enumeration (name, shape, kind)
# --------------------------------------------------------------------------------------
def _resnet(spec, pfx, cin, cout, temb):
    spec += [(pfx + ".norm1.weight", (cin,), "gain"), (pfx + ".norm1.bias", (cin,), "bias"),
             (pfx + ".conv1.weight", (cout, cin, 3, 3), "w"), (pfx + ".conv1.bias", (cout,), "bias")]
    if temb:
        spec += [(pfx + ".time_emb_proj.weight", (cout, temb), "w"), (pfx + ".time_emb_proj.bias", (cout,), "bias")]
    spec += [(pfx + ".norm2.weight", (cout,), "gain"), (pfx + ".norm2.bias", (cout,), "bias"),
             (pfx + ".conv2.weight", (cout, cout, 3, 3), "w"), (pfx + ".conv2.bias", (cout,), "bias")]
    if cin != cout:
        spec += [(pfx + ".conv_shortcut.weight", (cout, cin, 1, 1), "w"), (pfx + ".conv_shortcut.bias", (cout,), "bias")]


def _transformer(spec, pfx, c, ctx, depth=1, linear_proj=False):
    pshape = (c, c) if linear_proj else (c, c, 1, 1)
    spec += [(pfx + ".norm.weight", (c,), "gain"), (pfx + ".norm.bias", (c,), "bias"),
             (pfx + ".proj_in.weight", pshape, "w"), (pfx + ".proj_in.bias", (c,), "bias")]
    for d in range(depth):
        t = f"{pfx}.transformer_blocks.{d}"
        for n in ("norm1", "norm2", "norm3"):
            spec += [(f"{t}.{n}.weight", (c,), "gain"), (f"{t}.{n}.bias", (c,), "bias")]
        for a, kd in (("attn1", c), ("attn2", ctx)):
            spec += [(f"{t}.{a}.to_q.weight", (c, c), "w"), (f"{t}.{a}.to_k.weight", (c, kd), "w"),
                     (f"{t}.{a}.to_v.weight", (c, kd), "w"), (f"{t}.{a}.to_out.0.weight", (c, c), "w"),
                     (f"{t}.{a}.to_out.0.bias", (c,), "bias")]
        spec += [(f"{t}.ff.net.0.proj.weight", (8 * c, c), "w"), (f"{t}.ff.net.0.proj.bias", (8 * c,), "bias"),
                 (f"{t}.ff.net.2.weight", (c, 4 * c), "w"), (f"{t}.ff.net.2.bias", (c,), "bias")]
    spec += [(pfx + ".proj_out.weight", pshape, "w"), (pfx + ".proj_out.bias", (c,), "bias")]


def level_depth(cfg, i):
    """Transformer depth of level i (SD-1.5: 1 everywhere; SDXL: transformer_layers_per_block)."""
    return cfg["depth"][i] if "depth" in cfg else 1


def _encoder(spec, cfg):
    bo = cfg["block_out"]
    temb = cfg["temb_dim"]
    spec += [("conv_in.weight", (bo[0], cfg["in_channels"], 3, 3), "w"), ("conv_in.bias", (bo[0],), "bias"),
             ("time_embedding.linear_1.weight", (temb, bo[0]), "w"), ("time_embedding.linear_1.bias", (temb,), "bias"),
             ("time_embedding.linear_2.weight", (temb, temb), "w"), ("time_embedding.linear_2.bias", (temb,), "bias")]
    if "add_embed" in cfg:   # SDXL addition_embed_type "text_time"
        ae = cfg["add_embed"]
        ain = ae["n_ids"] * ae["time_dim"] + ae["pooled_dim"]
        spec += [("add_embedding.linear_1.weight", (temb, ain), "w"), ("add_embedding.linear_1.bias", (temb,), "bias"),
                 ("add_embedding.linear_2.weight", (temb, temb), "w"), ("add_embedding.linear_2.bias", (temb,), "bias")]
    lp = cfg.get("linear_proj", False)
    cin = bo[0]
    skip_ch = [bo[0]]
    for i, c in enumerate(bo):
        for j in range(cfg["layers"]):
            _resnet(spec, f"down_blocks.{i}.resnets.{j}", cin, c, temb)
            if cfg["attn"][i]:
                _transformer(spec, f"down_blocks.{i}.attentions.{j}", c, cfg["ctx_dim"], level_depth(cfg, i), lp)
            cin = c
            skip_ch.append(c)
        if i != len(bo) - 1:
            spec += [(f"down_blocks.{i}.downsamplers.0.conv.weight", (c, c, 3, 3), "w"),
                     (f"down_blocks.{i}.downsamplers.0.conv.bias", (c,), "bias")]
            skip_ch.append(c)
    _resnet(spec, "mid_block.resnets.0", cin, cin, temb)
    _transformer(spec, "mid_block.attentions.0", cin, cfg["ctx_dim"], level_depth(cfg, len(bo) - 1), lp)
    _resnet(spec, "mid_block.resnets.1", cin, cin, temb)
    return skip_ch


def unet_spec(cfg):
    spec = []
    skip_ch = _encoder(spec, cfg)
    bo = cfg["block_out"]
    rev = list(reversed(bo))
    rev_attn = list(reversed(cfg["attn"]))
    prev = rev[0]
    for i, c in enumerate(rev):
        for j in range(cfg["layers"] + 1):
            skip = skip_ch.pop()
            _resnet(spec, f"up_blocks.{i}.resnets.{j}", prev + skip, c, cfg["temb_dim"])
            if rev_attn[i]:
                _transformer(spec, f"up_blocks.{i}.attentions.{j}", c, cfg["ctx_dim"], level_depth(cfg, len(bo) - 1 - i),
                             cfg.get("linear_proj", False))
            prev = c
        if i != len(bo) - 1:
            spec += [(f"up_blocks.{i}.upsamplers.0.conv.weight", (c, c, 3, 3), "w"),
                     (f"up_blocks.{i}.upsamplers.0.conv.bias", (c,), "bias")]
    spec += [("conv_norm_out.weight", (bo[0],), "gain"), ("conv_norm_out.bias", (bo[0],), "bias"),
             ("conv_out.weight", (cfg["out_channels"], bo[0], 3, 3), "w"), ("conv_out.bias", (cfg["out_channels"],), "bias")]
    return spec


def controlnet_spec(cfg):
    spec = []
    skip_ch = _encoder(spec, cfg)
    ce = cfg["cond_embed"]
    p = "controlnet_cond_embedding"
    spec += [(p + ".conv_in.weight", (ce[0], cfg["cond_channels"], 3, 3), "w"), (p + ".conv_in.bias", (ce[0],), "bias")]
    for i in range(len(ce) - 1):
        spec += [(f"{p}.blocks.{2 * i}.weight", (ce[i], ce[i], 3, 3), "w"), (f"{p}.blocks.{2 * i}.bias", (ce[i],), "bias"),
                 (f"{p}.blocks.{2 * i + 1}.weight", (ce[i + 1], ce[i], 3, 3), "w"),
                 (f"{p}.blocks.{2 * i + 1}.bias", (ce[i + 1],), "bias")]
    bo = cfg["block_out"]
    spec += [(p + ".conv_out.weight", (bo[0], ce[-1], 3, 3), "w"), (p + ".conv_out.bias", (bo[0],), "bias")]
    for i, c in enumerate(skip_ch):
        spec += [(f"controlnet_down_blocks.{i}.weight", (c, c, 1, 1), "w"), (f"controlnet_down_blocks.{i}.bias", (c,), "bias")]
    spec += [("controlnet_mid_block.weight", (bo[-1], bo[-1], 1, 1), "w"), ("controlnet_mid_block.bias", (bo[-1],), "bias")]
    return spec


def vae_decoder_spec(cfg):
    spec = []
    lc = cfg["latent_channels"]
    bo = cfg["block_out"]
    top = bo[-1]
    spec += [("post_quant_conv.weight", (lc, lc, 1, 1), "w"), ("post_quant_conv.bias", (lc,), "bias"),
             ("decoder.conv_in.weight", (top, lc, 3, 3), "w"), ("decoder.conv_in.bias", (top,), "bias")]
    _resnet(spec, "decoder.mid_block.resnets.0", top, top, 0)
    a = "decoder.mid_block.attentions.0"
    spec += [(a + ".group_norm.weight", (top,), "gain"), (a + ".group_norm.bias", (top,), "bias")]
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        spec += [(f"{a}.{n}.weight", (top, top), "w"), (f"{a}.{n}.bias", (top,), "bias")]
    _resnet(spec, "decoder.mid_block.resnets.1", top, top, 0)
    prev = top
    for i, c in enumerate(reversed(bo)):
        for j in range(cfg["layers"] + 1):
            _resnet(spec, f"decoder.up_blocks.{i}.resnets.{j}", prev, c, 0)
            prev = c
        if i != len(bo) - 1:
            spec += [(f"decoder.up_blocks.{i}.upsamplers.0.conv.weight", (c, c, 3, 3), "w"),
                     (f"decoder.up_blocks.{i}.upsamplers.0.conv.bias", (c,), "bias")]
    spec += [("decoder.conv_norm_out.weight", (bo[0],), "gain"), ("decoder.conv_norm_out.bias", (bo[0],), "bias"),
             ("decoder.conv_out.weight", (cfg["out_channels"], bo[0], 3, 3), "w"),
             ("decoder.conv_out.bias", (cfg["out_channels"],), "bias")]
    return spec


def vae_encoder_spec(cfg):
    """AutoencoderKL encoder half + quant_conv (same checkpoint file as the decoder; SDEdit / img2img needs it)."""
    spec = []
    lc = cfg["latent_channels"]
    bo = cfg["block_out"]
    spec += [("encoder.conv_in.weight", (bo[0], cfg["out_channels"], 3, 3), "w"), ("encoder.conv_in.bias", (bo[0],), "bias")]
    prev = bo[0]
    for i, c in enumerate(bo):
        for j in range(cfg["layers"]):
            _resnet(spec, f"encoder.down_blocks.{i}.resnets.{j}", prev, c, 0)
            prev = c
        if i != len(bo) - 1:
            spec += [(f"encoder.down_blocks.{i}.downsamplers.0.conv.weight", (c, c, 3, 3), "w"),
                     (f"encoder.down_blocks.{i}.downsamplers.0.conv.bias", (c,), "bias")]
    top = bo[-1]
    _resnet(spec, "encoder.mid_block.resnets.0", top, top, 0)
    a = "encoder.mid_block.attentions.0"
    spec += [(a + ".group_norm.weight", (top,), "gain"), (a + ".group_norm.bias", (top,), "bias")]
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        spec += [(f"{a}.{n}.weight", (top, top), "w"), (f"{a}.{n}.bias", (top,), "bias")]
    _resnet(spec, "encoder.mid_block.resnets.1", top, top, 0)
    spec += [("encoder.conv_norm_out.weight", (top,), "gain"), ("encoder.conv_norm_out.bias", (top,), "bias"),
             ("encoder.conv_out.weight", (2 * lc, top, 3, 3), "w"), ("encoder.conv_out.bias", (2 * lc,), "bias"),
             ("quant_conv.weight", (2 * lc, 2 * lc, 1, 1), "w"), ("quant_conv.bias", (2 * lc,), "bias")]
    return spec


def clip_text_spec(cfg):
    w = cfg["width"]
    spec = [("text_model.embeddings.token_embedding.weight", (cfg["vocab"], w), "embed"),
            ("text_model.embeddings.position_embedding.weight", (cfg["max_pos"], w), "embed")]
    for i in range(cfg["layers"]):
        lp = f"text_model.encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            spec += [(f"{lp}.self_attn.{n}.weight", (w, w), "w"), (f"{lp}.self_attn.{n}.bias", (w,), "bias")]
        spec += [(f"{lp}.layer_norm1.weight", (w,), "gain"), (f"{lp}.layer_norm1.bias", (w,), "bias"),
                 (f"{lp}.mlp.fc1.weight", (cfg["mlp"], w), "w"), (f"{lp}.mlp.fc1.bias", (cfg["mlp"],), "bias"),
                 (f"{lp}.mlp.fc2.weight", (w, cfg["mlp"]), "w"), (f"{lp}.mlp.fc2.bias", (w,), "bias"),
                 (f"{lp}.layer_norm2.weight", (w,), "gain"), (f"{lp}.layer_norm2.bias", (w,), "bias")]
    spec += [("text_model.final_layer_norm.weight", (w,), "gain"), ("text_model.final_layer_norm.bias", (w,), "bias")]
    if "proj_dim" in cfg:    # CLIPTextModelWithProjection (SDXL text_encoder_2)
        spec += [("text_projection.weight", (cfg["proj_dim"], w), "w")]
    return spec


def blip2_qformer_spec(cfg):
    """Blip2QFormerModel of the BLIP-Diffusion repos (diffusers pipelines/blip_diffusion/modeling_blip2.py key names,
    recalled): vision tower, learned queries, BERT embeddings / layers with per-layer cross-attention and separate
    query / text feed-forwards, ProjLayer."""
    vw, w = cfg["vis_width"], cfg["width"]
    npos = (cfg["image_size"] // cfg["patch"]) ** 2 + 1
    v = "visual_encoder"
    spec = [(v + ".embeddings.class_embedding", (1, 1, vw), "embed"),
            (v + ".embeddings.patch_embedding.weight", (vw, 3, cfg["patch"], cfg["patch"]), "w"),
            (v + ".embeddings.position_embedding", (1, npos, vw), "embed"),
            (v + ".pre_layernorm.weight", (vw,), "gain"), (v + ".pre_layernorm.bias", (vw,), "bias")]
    for i in range(cfg["vis_layers"]):
        lp = f"{v}.encoder.layers.{i}"
        spec += [(lp + ".layer_norm1.weight", (vw,), "gain"), (lp + ".layer_norm1.bias", (vw,), "bias"),
                 (lp + ".self_attn.qkv.weight", (3 * vw, vw), "w"), (lp + ".self_attn.qkv.bias", (3 * vw,), "bias"),
                 (lp + ".self_attn.projection.weight", (vw, vw), "w"), (lp + ".self_attn.projection.bias", (vw,), "bias"),
                 (lp + ".layer_norm2.weight", (vw,), "gain"), (lp + ".layer_norm2.bias", (vw,), "bias"),
                 (lp + ".mlp.fc1.weight", (cfg["vis_mlp"], vw), "w"), (lp + ".mlp.fc1.bias", (cfg["vis_mlp"],), "bias"),
                 (lp + ".mlp.fc2.weight", (vw, cfg["vis_mlp"]), "w"), (lp + ".mlp.fc2.bias", (vw,), "bias")]
    spec += [(v + ".post_layernorm.weight", (vw,), "gain"), (v + ".post_layernorm.bias", (vw,), "bias"),
             ("query_tokens", (1, cfg["num_query"], w), "embed"),
             ("embeddings.word_embeddings.weight", (cfg["vocab"], w), "embed"),
             ("embeddings.position_embeddings.weight", (cfg["max_pos"], w), "embed"),
             ("embeddings.LayerNorm.weight", (w,), "gain"), ("embeddings.LayerNorm.bias", (w,), "bias")]

    def dense_ln(pfx, cin, cout):
        return [(pfx + ".dense.weight", (cout, cin), "w"), (pfx + ".dense.bias", (cout,), "bias"),
                (pfx + ".LayerNorm.weight", (cout,), "gain"), (pfx + ".LayerNorm.bias", (cout,), "bias")]

    for i in range(cfg["layers"]):
        lp = f"encoder.layer.{i}"
        for n in ("query", "key", "value"):
            spec += [(f"{lp}.attention.attention.{n}.weight", (w, w), "w"), (f"{lp}.attention.attention.{n}.bias", (w,), "bias")]
        spec += dense_ln(lp + ".attention.output", w, w)
        if i % cfg["cross_freq"] == 0:
            spec += [(f"{lp}.crossattention.attention.query.weight", (w, w), "w"), (f"{lp}.crossattention.attention.query.bias", (w,), "bias")]
            for n in ("key", "value"):
                spec += [(f"{lp}.crossattention.attention.{n}.weight", (w, vw), "w"), (f"{lp}.crossattention.attention.{n}.bias", (w,), "bias")]
            spec += dense_ln(lp + ".crossattention.output", w, w)
        for sfx in ("", "_query"):
            spec += [(f"{lp}.intermediate{sfx}.dense.weight", (cfg["mlp"], w), "w"), (f"{lp}.intermediate{sfx}.dense.bias", (cfg["mlp"],), "bias")]
            spec += dense_ln(f"{lp}.output{sfx}", cfg["mlp"], w)
    spec += [("proj_layer.dense1.weight", (cfg["proj_hidden"], w), "w"), ("proj_layer.dense1.bias", (cfg["proj_hidden"],), "bias"),
             ("proj_layer.dense2.weight", (cfg["out_dim"], cfg["proj_hidden"]), "w"), ("proj_layer.dense2.bias", (cfg["out_dim"],), "bias"),
             ("proj_layer.LayerNorm.weight", (w,), "gain"), ("proj_layer.LayerNorm.bias", (w,), "bias")]
    return spec


def safety_checker_spec(cfg):
    """StableDiffusionSafetyChecker state dict (diffusers key names; "pre_layrnorm" is the checkpoint's spelling)."""
    w = cfg["width"]
    npos = (cfg["image_size"] // cfg["patch"]) ** 2 + 1
    v = "vision_model.vision_model"
    spec = [(v + ".embeddings.class_embedding", (w,), "embed"),
            (v + ".embeddings.patch_embedding.weight", (w, 3, cfg["patch"], cfg["patch"]), "w"),
            (v + ".embeddings.position_embedding.weight", (npos, w), "embed"),
            (v + ".pre_layrnorm.weight", (w,), "gain"), (v + ".pre_layrnorm.bias", (w,), "bias")]
    for i in range(cfg["layers"]):
        lp = f"{v}.encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            spec += [(f"{lp}.self_attn.{n}.weight", (w, w), "w"), (f"{lp}.self_attn.{n}.bias", (w,), "bias")]
        spec += [(f"{lp}.layer_norm1.weight", (w,), "gain"), (f"{lp}.layer_norm1.bias", (w,), "bias"),
                 (f"{lp}.mlp.fc1.weight", (cfg["mlp"], w), "w"), (f"{lp}.mlp.fc1.bias", (cfg["mlp"],), "bias"),
                 (f"{lp}.mlp.fc2.weight", (w, cfg["mlp"]), "w"), (f"{lp}.mlp.fc2.bias", (w,), "bias"),
                 (f"{lp}.layer_norm2.weight", (w,), "gain"), (f"{lp}.layer_norm2.bias", (w,), "bias")]
    spec += [(v + ".post_layernorm.weight", (w,), "gain"), (v + ".post_layernorm.bias", (w,), "bias"),
             ("visual_projection.weight", (cfg["proj_dim"], w), "w"),
             ("concept_embeds", (cfg["n_concepts"], cfg["proj_dim"]), "embed"),
             ("special_care_embeds", (cfg["n_special"], cfg["proj_dim"]), "embed"),
             ("concept_embeds_weights", (cfg["n_concepts"],), "thresh"),
             ("special_care_embeds_weights", (cfg["n_special"],), "thresh")]
    return spec


def blip_caption_spec(cfg):
    """The BLIP captioner (config.BLIP_CAPTION) under the key names of transformers' BlipForConditionalGeneration: vision_model.*,
    text_decoder.bert.*, text_decoder.cls.predictions.* -- the one layout a test pins.  (The LM-head decoder weight is tied to the
    word embeddings in the trained model; a synthetic state dict draws its own.)"""
    vw, w = cfg["vis_width"], cfg["width"]
    npos = (cfg["image_size"] // cfg["patch"]) ** 2 + 1
    v = "vision_model"
    spec = [(v + ".embeddings.class_embedding", (1, 1, vw), "embed"),
            (v + ".embeddings.position_embedding", (1, npos, vw), "embed"),
            (v + ".embeddings.patch_embedding.weight", (vw, 3, cfg["patch"], cfg["patch"]), "w"),
            (v + ".embeddings.patch_embedding.bias", (vw,), "bias")]
    for i in range(cfg["vis_layers"]):
        lp = f"{v}.encoder.layers.{i}"
        spec += [(lp + ".self_attn.qkv.weight", (3 * vw, vw), "w"), (lp + ".self_attn.qkv.bias", (3 * vw,), "bias"),
                 (lp + ".self_attn.projection.weight", (vw, vw), "w"), (lp + ".self_attn.projection.bias", (vw,), "bias"),
                 (lp + ".layer_norm1.weight", (vw,), "gain"), (lp + ".layer_norm1.bias", (vw,), "bias"),
                 (lp + ".mlp.fc1.weight", (cfg["vis_mlp"], vw), "w"), (lp + ".mlp.fc1.bias", (cfg["vis_mlp"],), "bias"),
                 (lp + ".mlp.fc2.weight", (vw, cfg["vis_mlp"]), "w"), (lp + ".mlp.fc2.bias", (vw,), "bias"),
                 (lp + ".layer_norm2.weight", (vw,), "gain"), (lp + ".layer_norm2.bias", (vw,), "bias")]
    spec += [(v + ".post_layernorm.weight", (vw,), "gain"), (v + ".post_layernorm.bias", (vw,), "bias")]
    b = "text_decoder.bert"
    spec += [(b + ".embeddings.word_embeddings.weight", (cfg["vocab"], w), "embed"),
             (b + ".embeddings.position_embeddings.weight", (cfg["max_pos"], w), "embed"),
             (b + ".embeddings.LayerNorm.weight", (w,), "gain"), (b + ".embeddings.LayerNorm.bias", (w,), "bias")]

    def dense_ln(pfx, cin, cout):
        return [(pfx + ".dense.weight", (cout, cin), "w"), (pfx + ".dense.bias", (cout,), "bias"),
                (pfx + ".LayerNorm.weight", (cout,), "gain"), (pfx + ".LayerNorm.bias", (cout,), "bias")]

    for i in range(cfg["layers"]):
        lp = f"{b}.encoder.layer.{i}"
        for a, kin in (("attention", w), ("crossattention", vw)):
            spec += [(f"{lp}.{a}.self.query.weight", (w, w), "w"), (f"{lp}.{a}.self.query.bias", (w,), "bias")]
            for n in ("key", "value"):
                spec += [(f"{lp}.{a}.self.{n}.weight", (w, kin), "w"), (f"{lp}.{a}.self.{n}.bias", (w,), "bias")]
            spec += dense_ln(f"{lp}.{a}.output", w, w)
        spec += [(f"{lp}.intermediate.dense.weight", (cfg["mlp"], w), "w"), (f"{lp}.intermediate.dense.bias", (cfg["mlp"],), "bias")]
        spec += dense_ln(f"{lp}.output", cfg["mlp"], w)
    c = "text_decoder.cls.predictions"
    spec += dense_ln(c + ".transform", w, w)
    spec += [(c + ".decoder.weight", (cfg["vocab"], w), "w"), (c + ".decoder.bias", (cfg["vocab"],), "bias")]
    return spec


def blip_caption_from_transformers(sd):
    """A BlipForConditionalGeneration state dict -> the names of blip_caption_spec, fp32: buffers (position_ids) dropped, the tied
    copies resolved (cls.predictions.bias is decoder.bias; a file saved without the tied decoder weight takes the word embeddings)."""
    c = "text_decoder.cls.predictions"
    out = {k: v.detach().float() for k, v in sd.items() if not k.endswith("position_ids") and k != c + ".bias"}
    if c + ".decoder.bias" not in out and c + ".bias" in sd:
        out[c + ".decoder.bias"] = sd[c + ".bias"].detach().float()
    if c + ".decoder.weight" not in out:
        out[c + ".decoder.weight"] = out["text_decoder.bert.embeddings.word_embeddings.weight"]
    return out


# LAVIS BlipCaption checkpoint (model_base_caption_capfilt_large.pth, under its "model" entry): the timm-style ViT names of
# lavis/models/vit.py.  RECALLED, UNVERIFIED: no LAVIS checkpoint could be read here; a wrong name fails loudly (KeyError at pack time).
_LAVIS_VIT = (("visual_encoder.cls_token", "vision_model.embeddings.class_embedding"),
              ("visual_encoder.pos_embed", "vision_model.embeddings.position_embedding"),
              ("visual_encoder.patch_embed.proj.", "vision_model.embeddings.patch_embedding."),
              ("visual_encoder.norm.", "vision_model.post_layernorm."))
_LAVIS_BLOCK = ((".norm1.", ".layer_norm1."), (".norm2.", ".layer_norm2."), (".attn.qkv.", ".self_attn.qkv."),
                (".attn.proj.", ".self_attn.projection."))


def blip_caption_from_lavis(sd):
    """A LAVIS BlipCaption state dict (visual_encoder.*, text_decoder.*) -> the names of blip_caption_spec.  Key names recalled, unverified."""
    sd = sd.get("model", sd)
    out = {}
    for k, v in sd.items():
        if k.startswith("visual_encoder.blocks."):
            k = k.replace("visual_encoder.blocks.", "vision_model.encoder.layers.", 1)
            for a, b in _LAVIS_BLOCK:
                k = k.replace(a, b, 1)
        else:
            for a, b in _LAVIS_VIT:
                if k.startswith(a):
                    k = b + k[len(a):]
                    break
        out[k] = v
    return blip_caption_from_transformers(out)


def t5_keys(cfg):
    """[(name, shape, kind)] of a T5 v1.0 encoder-decoder in the public transformers layout (T5ForConditionalGeneration.state_dict()
    without the tied copies encoder.embed_tokens / decoder.embed_tokens): no biases anywhere, the relative-position table in block 0
    of each stack only.  kind: "emb" | "q" | "w" (other projections; fan-in = shape[1]) | "rel" | "gain" | "gain_out"."""
    d, inner, ff = cfg["d_model"], cfg["heads"] * cfg["d_kv"], cfg["d_ff"]
    spec = [("shared.weight", (cfg["vocab"], d), "emb")]

    def attn(pfx, rel):
        out = [(f"{pfx}.q.weight", (inner, d), "q"), (f"{pfx}.k.weight", (inner, d), "w"), (f"{pfx}.v.weight", (inner, d), "w"),
               (f"{pfx}.o.weight", (d, inner), "w")]
        return out + ([(f"{pfx}.relative_attention_bias.weight", (cfg["buckets"], cfg["heads"]), "rel")] if rel else [])

    for stack, layers in (("encoder", cfg["enc_layers"]), ("decoder", cfg["dec_layers"])):
        for i in range(layers):
            b = f"{stack}.block.{i}.layer"
            spec += attn(f"{b}.0.SelfAttention", i == 0) + [(f"{b}.0.layer_norm.weight", (d,), "gain")]
            j = 1
            if stack == "decoder":
                spec += attn(f"{b}.1.EncDecAttention", False) + [(f"{b}.1.layer_norm.weight", (d,), "gain")]
                j = 2
            spec += [(f"{b}.{j}.DenseReluDense.wi.weight", (ff, d), "w"), (f"{b}.{j}.DenseReluDense.wo.weight", (d, ff), "w"),
                     (f"{b}.{j}.layer_norm.weight", (d,), "gain")]
        spec.append((f"{stack}.final_layer_norm.weight", (d,), "gain_out" if stack == "decoder" else "gain"))
    if not cfg["tie_embeddings"]:
        spec.append(("lm_head.weight", (cfg["vocab"], d), "emb"))
    return spec


def t5_synth_state_dict(cfg, seed=0):
    """Seeded synthetic T5 weights in the public key layout.  NOT transformers' default init: with it (embeddings of std 1, projections
    scaled down by a further d_kv ** -0.5) the residual stream of a shallow model is its start token's embedding, the tied LM head
    reads that embedding back, and the tiny model emits id 0 for ever.  Chosen instead: every projection at unit gain (std =
    fan_in ** -0.5, q included: T5 has no 1 / sqrt(d_kv) in its logits, so attention is sharp), embeddings of std 0.05 (the sub-layers'
    outputs, not the token's own embedding, dominate the stream: at 0.25 the tied head still reads the last token back and greedy
    sequences repeat it), relative-position tables of std 1, norm gains 1 +- 0.1, and the decoder's final gain around 40 so that
    the logits spread over a few units -- greedy and sampled sequences then vary with the input and from step to step."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape, kind in t5_keys(cfg):
        r = torch.randn(shape, generator=g)
        if kind == "emb":
            sd[name] = 0.05 * r
        elif kind in ("q", "w"):
            sd[name] = r * shape[1] ** -0.5
        elif kind == "rel":
            sd[name] = r
        else:
            sd[name] = (40.0 if kind == "gain_out" else 1.0) * (1.0 + 0.1 * r)
    return sd


def t5_from_hf(sd, cfg):
    """A T5ForConditionalGeneration state dict (public layout) -> fp32 tensors under the names of t5_keys: the tied copies
    (encoder.embed_tokens / decoder.embed_tokens, and lm_head under tied embeddings) dropped, every expected name and shape checked --
    a missing or misshapen tensor raises here, not at pack time."""
    out = {}
    for name, shape, _ in t5_keys(cfg):
        if name not in sd:
            raise KeyError(f"T5 checkpoint lacks {name}")
        t = sd[name].detach().float()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"T5 checkpoint: {name} is {tuple(t.shape)}, the config says {tuple(shape)}")
        out[name] = t.contiguous()
    return out


SPECS = dict(blip_caption=blip_caption_spec, safety=safety_checker_spec, unet=unet_spec, controlnet=controlnet_spec, vae=vae_decoder_spec, text=clip_text_spec, text2=clip_text_spec,
             qformer=blip2_qformer_spec)


def _bn(spec, pfx, c):
    spec += [(pfx + ".weight", (c,), "gain"), (pfx + ".bias", (c,), "bias"), (pfx + ".running_mean", (c,), "bias"),
             (pfx + ".running_var", (c,), "var")]


def clip_rn50_spec(cfg):
    """OpenAI CLIP RN50 state dict (ModifiedResNet + AttentionPool2d under `visual.`, text transformer, projections)."""
    spec = []
    w = cfg["width"]
    v = "visual"
    for i, (ci, co) in enumerate(((3, w // 2), (w // 2, w // 2), (w // 2, w))):
        spec.append((f"{v}.conv{i + 1}.weight", (co, ci, 3, 3), "w"))
        _bn(spec, f"{v}.bn{i + 1}", co)
    inpl = w
    for li, nb in enumerate(cfg["layers"]):
        planes = w * (2 ** li)
        for bi in range(nb):
            pf = f"{v}.layer{li + 1}.{bi}"
            stride = 2 if (bi == 0 and li > 0) else 1
            spec.append((pf + ".conv1.weight", (planes, inpl, 1, 1), "w"))
            _bn(spec, pf + ".bn1", planes)
            spec.append((pf + ".conv2.weight", (planes, planes, 3, 3), "w"))
            _bn(spec, pf + ".bn2", planes)
            spec.append((pf + ".conv3.weight", (planes * 4, planes, 1, 1), "w"))
            _bn(spec, pf + ".bn3", planes * 4)
            if stride > 1 or inpl != planes * 4:
                spec.append((pf + ".downsample.0.weight", (planes * 4, inpl, 1, 1), "w"))
                _bn(spec, pf + ".downsample.1", planes * 4)
            inpl = planes * 4
    a = v + ".attnpool"
    sp = (cfg["image_size"] // 32) ** 2 + 1
    spec.append((a + ".positional_embedding", (sp, inpl), "pos"))
    for n, co in (("q_proj", inpl), ("k_proj", inpl), ("v_proj", inpl), ("c_proj", cfg["embed_dim"])):
        spec += [(f"{a}.{n}.weight", (co, inpl), "w"), (f"{a}.{n}.bias", (co,), "bias")]
    tw = cfg["text_width"]
    spec += [("token_embedding.weight", (cfg["vocab"], tw), "emb"), ("positional_embedding", (cfg["context"], tw), "pos")]
    for i in range(cfg["text_layers"]):
        pf = f"transformer.resblocks.{i}"
        spec += [(pf + ".attn.in_proj_weight", (3 * tw, tw), "w"), (pf + ".attn.in_proj_bias", (3 * tw,), "bias"),
                 (pf + ".attn.out_proj.weight", (tw, tw), "w"), (pf + ".attn.out_proj.bias", (tw,), "bias"),
                 (pf + ".ln_1.weight", (tw,), "gain"), (pf + ".ln_1.bias", (tw,), "bias"),
                 (pf + ".ln_2.weight", (tw,), "gain"), (pf + ".ln_2.bias", (tw,), "bias"),
                 (pf + ".mlp.c_fc.weight", (4 * tw, tw), "w"), (pf + ".mlp.c_fc.bias", (4 * tw,), "bias"),
                 (pf + ".mlp.c_proj.weight", (tw, 4 * tw), "w"), (pf + ".mlp.c_proj.bias", (tw,), "bias")]
    spec += [("ln_final.weight", (tw,), "gain"), ("ln_final.bias", (tw,), "bias"),
             ("text_projection", (tw, cfg["embed_dim"]), "wt"), ("logit_scale", (), "logit_scale")]
    return spec


def wsdan_cal_spec(cfg):
    """WSDAN_CAL state dict (fgvc/models/cal.py:131-166): `features` = Sequential(conv1, bn1, relu, maxpool, layer1..4) of the
    fgvc ResNet (keys features.0 / .1 / .4 .. .7), `attentions` = BasicConv2d (1x1 conv + BN), `fc` (no bias)."""
    spec = []
    w = cfg["width"]
    spec.append(("features.0.weight", (w, 3, 7, 7), "w"))
    _bn(spec, "features.1", w)
    inpl = w
    for li, nb in enumerate(cfg["layers"]):
        planes = w * (2 ** li)
        for bi in range(nb):
            pf = f"features.{4 + li}.{bi}"
            stride = (1, 2, 2, 1)[li] if bi == 0 else 1      # layer4 unstrided (fgvc ResNet stride=1)
            spec.append((pf + ".conv1.weight", (planes, inpl, 1, 1), "w"))
            _bn(spec, pf + ".bn1", planes)
            spec.append((pf + ".conv2.weight", (planes, planes, 3, 3), "w"))
            _bn(spec, pf + ".bn2", planes)
            spec.append((pf + ".conv3.weight", (planes * 4, planes, 1, 1), "w"))
            _bn(spec, pf + ".bn3", planes * 4)
            if stride != 1 or inpl != planes * 4:
                spec.append((pf + ".downsample.0.weight", (planes * 4, inpl, 1, 1), "w"))
                _bn(spec, pf + ".downsample.1", planes * 4)
            inpl = planes * 4
    m = cfg["attentions"]
    spec.append(("attentions.conv.weight", (m, inpl, 1, 1), "w"))
    _bn(spec, "attentions.bn", m)
    spec.append(("fc.weight", (cfg["num_classes"], m * inpl), "w_fc"))
    return spec


def hed_spec(cfg):
    """ControlNetHED.pth (controlnet_aux `ControlNetHED_Apache2`): `norm` [1,3,1,1], `block{i}.convs.{j}.{weight,bias}`,
    `block{i}.projection.{weight,bias}`."""
    spec = [("norm", (1, 3, 1, 1), "hed_norm")]
    prev = 3
    for i, (c, n) in enumerate(cfg["blocks"]):
        for j in range(n):
            spec += [(f"block{i + 1}.convs.{j}.weight", (c, prev if j == 0 else c, 3, 3), "w"), (f"block{i + 1}.convs.{j}.bias", (c,), "bias")]
        spec += [(f"block{i + 1}.projection.weight", (1, c, 1, 1), "w"), (f"block{i + 1}.projection.bias", (1,), "bias")]
        prev = c
    return spec


LPIPS_ALEX_CONVS = ((0, 11), (3, 5), (6, 3), (8, 3), (10, 3))      # (index in torchvision AlexNet.features, window)


def lpips_alex_spec(cfg):
    """torchvision AlexNet `features.{0,3,6,8,10}.{weight,bias}` + lpips v0.1 `lin{0..4}.model.1.weight` ([1, C, 1, 1], >= 0)."""
    spec, cin = [], 3
    for (idx, k), co in zip(LPIPS_ALEX_CONVS, cfg["channels"]):
        spec += [(f"features.{idx}.weight", (co, cin, k, k), "w"), (f"features.{idx}.bias", (co,), "bias")]
        cin = co
    spec += [(f"lin{i}.model.1.weight", (1, c, 1, 1), "lin") for i, c in enumerate(cfg["channels"])]
    return spec


SPECS.update(clip_rn50=clip_rn50_spec, cal=wsdan_cal_spec, vae_enc=vae_encoder_spec, hed=hed_spec, lpips_alex=lpips_alex_spec)


def fold_bn(conv_w, sd, bn_pfx, eps=1e-5):
    """Inference BatchNorm folded into the preceding bias-free conv: (w * s[:, None, None, None], beta - mean * s) with
    s = gamma / sqrt(var + eps) -- computed in fp64, stored fp32."""
    g, b = sd[bn_pfx + ".weight"].double(), sd[bn_pfx + ".bias"].double()
    m, v = sd[bn_pfx + ".running_mean"].double(), sd[bn_pfx + ".running_var"].double()
    s = g / torch.sqrt(v + eps)
    return (conv_w.double() * s.reshape(-1, *([1] * (conv_w.dim() - 1)))).float(), (b - m * s).float()


def openai_clip_text_to_hf(sd, layers):
    """OpenAI CLIP text-tower keys (transformer.resblocks.N.attn.in_proj_weight ...) -> the transformers names the CLIPText
    launch graph packs (text_model.encoder.layers.N.self_attn.q_proj.weight ...); text_projection is stored [width, embed]
    by OpenAI and applied as x @ P, i.e. the Linear weight is its transpose."""
    out = {"text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].t().contiguous()}
    for i in range(layers):
        a, b = f"transformer.resblocks.{i}", f"text_model.encoder.layers.{i}"
        wq, wk, wv = sd[a + ".attn.in_proj_weight"].chunk(3, dim=0)
        bq, bk, bv = sd[a + ".attn.in_proj_bias"].chunk(3, dim=0)
        for n, w_, b_ in (("q_proj", wq, bq), ("k_proj", wk, bk), ("v_proj", wv, bv)):
            out[f"{b}.self_attn.{n}.weight"], out[f"{b}.self_attn.{n}.bias"] = w_.contiguous(), b_.contiguous()
        out[b + ".self_attn.out_proj.weight"], out[b + ".self_attn.out_proj.bias"] = sd[a + ".attn.out_proj.weight"], sd[a + ".attn.out_proj.bias"]
        for src, dst in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[f"{b}.{dst}.weight"], out[f"{b}.{dst}.bias"] = sd[f"{a}.{src}.weight"], sd[f"{a}.{src}.bias"]
    return out


_BIG = 1 << 20          # elements: tensors at least this large are drawn chunk-wise on a thread pool
_BIG_EXEMPT = ("cal", "clip_rn50", "hed")     # kinds whose tensors stay on the sequential stream: reference goldens
                                              # (tests/golden/reference_filter_golden.json) were made from them
_BIG_SCALE = {"w": None, "pos": None, "wt": None, "w_fc": 0.05, "embed": 0.5}


def _fill_big(pending, seed):
    """Draw every large tensor of a state dict: rows are cut into chunks of <= 1 M elements, each from its own generator
    seeded by (state-dict seed, tensor index, chunk index), ALL chunks of all tensors on one thread pool -- torch's seeded
    CPU generator is serial (~30 M values/s), which made synthesising the 4.7 B parameters of the SDXL family take 100 s."""
    import concurrent.futures as cf
    import os
    jobs = []
    for index, t, scale in pending:
        flat = t.view(t.shape[0], -1)
        rows = max(1, (1 << 20) // max(1, flat.shape[1]))
        for j, r0 in enumerate(range(0, t.shape[0], rows)):
            jobs.append((flat, r0, min(t.shape[0], r0 + rows), (seed * 1000003 + index * 7919 + j * 104729 + 12345) & 0x7FFFFFFF, scale))

    def draw(job):
        flat, r0, r1, sd_, scale = job
        gj = torch.Generator().manual_seed(sd_)
        flat[r0:r1] = torch.randn((r1 - r0, flat.shape[1]), generator=gj) * scale

    # one process per GPU each synthesises its own copy (bench.py --gpus N, run_aug with SASPA_GPUS): the ranks of a node
    # share its cores, so every rank takes its share instead of 16 threads each (8 ranks x 16 threads in a 16-thread
    # cgroup spent the start-up thrashing); SASPA_SYNTH_THREADS overrides
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")) or 1))
    try:
        ncpu = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        ncpu = os.cpu_count() or 4
    # (synth_family_shared -- ONE drawing rank per node while the others wait in a collective -- lifts the share through
    # _SYNTH_THREADS_OVERRIDE, so that rank uses the node's whole allowance)
    workers = _SYNTH_THREADS_OVERRIDE[0] or int(os.environ.get("SASPA_SYNTH_THREADS", "0")) or max(1, min(16, ncpu // local_world))
    with cf.ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(draw, jobs, chunksize=1))


_SYNTH_THREADS_OVERRIDE = [0]     # thread count forced by synth_family_shared for the node's single drawing rank


def synth_state_dict(kind, cfg, seed=0):
    """Seeded synthetic fp32 state dict with diffusers key names."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    pending = []          # large tensors: allocated here, filled in parallel at the end
    for index, (name, shape, k) in enumerate(SPECS[kind](cfg)):
        numel = 1
        for d in shape:
            numel *= d
        if numel >= _BIG and k in _BIG_SCALE and len(shape) >= 2 and kind not in _BIG_EXEMPT:
            if k == "w":
                fan_in = 1
                for d in shape[1:]:
                    fan_in *= d
                scale = 1.0 / math.sqrt(fan_in)
            elif k == "pos":
                scale = 1.0 / math.sqrt(shape[-1])
            elif k == "wt":
                scale = 1.0 / math.sqrt(shape[0])
            else:
                scale = _BIG_SCALE[k]
            t = torch.empty(tuple(shape), dtype=torch.float32)
            pending.append((index, t, scale))
            sd[name] = t
            continue
        if k == "w":
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(fan_in))
        elif k == "gain":
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif k == "bias":
            t = 0.05 * torch.randn(shape, generator=g)
        elif k == "var":            # BatchNorm running variance: positive, around 1
            t = 0.5 + torch.rand(shape, generator=g)
        elif k == "pos":            # position tables of width shape[-1]
            t = torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        elif k == "wt":             # [in, out] projection applied as x @ P
            t = torch.randn(shape, generator=g) / math.sqrt(shape[0])
        elif k == "w_fc":           # classifier over unit-norm x 100 features: keeps the logits O(1) apart
            t = torch.randn(shape, generator=g) * 0.05
        elif k == "lin":            # LPIPS channel weights: non-negative
            t = torch.rand(shape, generator=g) * (2.0 / shape[1])
        elif k == "logit_scale":
            t = torch.tensor(math.log(100.0))
        elif k == "hed_norm":       # per-channel pixel mean on the 0..255 scale
            t = 110.0 + 20.0 * torch.rand(shape, generator=g)
        elif k == "thresh":
            # cosine thresholds of the safety checker (the real ones lie around 0.18-0.3): 6 sigma of the cosine of two
            # random proj_dim-vectors (0.217 at 768) so that random weights never flag an image by accident
            t = 6.0 / math.sqrt(cfg["proj_dim"]) + 0.01 * torch.randn(shape, generator=g)
        else:  # embeddings
            t = 0.5 * torch.randn(shape, generator=g)
        sd[name] = t
    if pending:
        _fill_big(pending, seed)
    return sd


def synth_family(cfgs, seed=0):
    kinds = ("unet", "controlnet", "vae", "text") + (("qformer",) if "qformer" in cfgs else ()) + \
        (("text2",) if "text2" in cfgs else ()) + (("safety",) if "safety" in cfgs else ())
    # (a family without a ControlNet -- config.IP2P -- keeps the other networks' seeds; any other missing network is a KeyError)
    fam = {k: synth_state_dict(k, cfgs[k], seed + i) for i, k in enumerate(kinds) if k != "controlnet" or k in cfgs}
    # the checkpoint's vae/ file holds encoder AND decoder: the encoder half (SDEdit / img2img) gets its own seed so the
    # decoder tensors are unchanged
    fam["vae"].update(synth_state_dict("vae_enc", cfgs["vae"], seed + 100))
    return fam


def synth_family_shared(cfgs, seed=0, dist=None, tag="family"):
    """`synth_family` for one-process-per-GPU jobs (bench.py --gpus N): the first rank of each node draws the family ONCE and
    parks it in /dev/shm; the other ranks of the node map that file (torch.load(mmap=True): shared pages, no second copy in
    RAM) instead of running N CPU synthesisers side by side in one cgroup.  The file is unlinked as soon as every rank has
    mapped it.  If any node cannot park the file (no /dev/shm, or one too small -- containers default to 64 MB), every rank
    falls back to drawing its own copy.  `dist`: an initialised torch.distributed module (None / world 1 -> plain synth_family)."""
    import os
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return synth_family(cfgs, seed)
    if "LOCAL_RANK" not in os.environ:
        # the global rank is NOT a stand-in: on a second node its ranks would wait for a file nobody wrote there
        raise RuntimeError("synth_family_shared: LOCAL_RANK must be set when the world has more than one rank "
                           "(torchrun and saspa_aug_amd/launcher.py both set it)")
    local_rank = int(os.environ["LOCAL_RANK"])
    path = os.path.join("/dev/shm", f"saspa_synth_{os.getuid()}_{os.environ.get('MASTER_PORT', '0')}_{tag}_{seed}.pt")
    fam, ok, err = None, True, None
    if local_rank == 0:
        try:
            # the only drawing rank of this node: the whole CPU allowance, not a 1/N share (the others idle in the collective)
            try:
                ncpu = len(os.sched_getaffinity(0))
            except (AttributeError, OSError):
                ncpu = os.cpu_count() or 4
            _SYNTH_THREADS_OVERRIDE[0] = int(os.environ.get("SASPA_SYNTH_THREADS", "0")) or max(1, min(16, ncpu))
            try:
                fam = synth_family(cfgs, seed)
            finally:
                _SYNTH_THREADS_OVERRIDE[0] = 0
            need = sum(t.numel() * t.element_size() for sd in fam.values() for t in sd.values())
            st = os.statvfs("/dev/shm")
            if st.f_bavail * st.f_frsize < need * 1.05 + (64 << 20):
                raise OSError(f"/dev/shm has {st.f_bavail * st.f_frsize >> 20} MB free, the family needs {need >> 20} MB")
            torch.save(fam, path + ".tmp")
            os.replace(path + ".tmp", path)
        except Exception as e:          # torch.save reports ENOSPC / short writes as RuntimeError; ANY failure must still
            ok = False                  # reach the collective below, or the other ranks hang until the backend's timeout
            if fam is None:
                err = e                 # the draw itself failed: re-raised after the collective
        finally:
            if not ok or os.path.exists(path + ".tmp"):
                for f in (path + ".tmp",) + (() if ok else (path,)):
                    try:
                        os.unlink(f)
                    except OSError:
                        pass
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)                      # also the "file is there" barrier
    if err is not None:
        raise err
    if not all(flags):                                     # some node could not park it: everyone draws its own
        if local_rank == 0 and ok:
            try:
                os.unlink(path)
            except OSError:
                pass
        return fam if fam is not None else synth_family(cfgs, seed)
    if fam is None:
        fam = torch.load(path, mmap=True, weights_only=True)
    dist.barrier()
    if local_rank == 0:
        try:
            os.unlink(path)
        except OSError:
            pass
    return fam


_LEGACY_ATTN_KEYS = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def remap_legacy_attention_keys(sd):
    """Checkpoints saved before diffusers 0.7 (runwayml/stable-diffusion-v1-5's `vae/`, `sd-vae-ft-mse`) carry the old
    `AttentionBlock` names `<attn>.query|key|value|proj_attn.{weight,bias}`; diffusers renames them at load time
    (`_convert_deprecated_attention_blocks`) to `to_q|to_k|to_v|to_out.0`.  Same remap here; 1x1-conv shaped weights
    ([C, C, 1, 1], the even older conv form) are squeezed to the Linear shape.  Keys already in the new form pass."""
    out = {}
    for k, v in sd.items():
        m = re.match(r"^(.*\.attentions\.\d+)\.(query|key|value|proj_attn)\.(weight|bias)$", k)
        if m:
            k = f"{m.group(1)}.{_LEGACY_ATTN_KEYS[m.group(2)]}.{m.group(3)}"
            if m.group(3) == "weight" and v.dim() == 4 and v.shape[2:] == (1, 1):
                v = v[:, :, 0, 0]
        elif re.match(r"^.*\.attentions\.\d+\.to_(q|k|v|out\.0)\.weight$", k) and v.dim() == 4 and v.shape[2:] == (1, 1):
            v = v[:, :, 0, 0]
        if k in out:
            raise KeyError(f"checkpoint holds both the legacy and the current name of {k}")
        out[k] = v
    return out


def load_safetensors(path):
    """Read a diffusers `*.safetensors` checkpoint into an fp32 state dict (legacy attention key names remapped)."""
    from safetensors.torch import load_file
    return remap_legacy_attention_keys({k: v.float() for k, v in load_file(path).items()})


# --------------------------------------------------------------------------------------
# packing into the kernel layout
# --------------------------------------------------------------------------------------
def round8(n):
    return (n + 7) // 8 * 8


def pack_conv(w, cin_pad=None):
    """[Cout, Cin, kh, kw] -> [Cout, kh*kw*Cin_pad] with K index (ky*kw+kx)*Cin_pad + c."""
    co, ci, kh, kw = w.shape
    cp = round8(ci) if cin_pad is None else cin_pad
    t = w.permute(0, 2, 3, 1)
    if cp != ci:
        t = torch.nn.functional.pad(t, (0, cp - ci))
    return t.reshape(co, kh * kw * cp).contiguous()


def pack_conv_split(w, c0, c0_pad, c1, c1_pad):
    """Conv over a channel concat [src0 (c0) | src1 (c1)] whose sources are stored padded."""
    co, ci, kh, kw = w.shape
    assert ci == c0 + c1
    t = w.permute(0, 2, 3, 1)
    a = torch.nn.functional.pad(t[..., :c0], (0, c0_pad - c0))
    b = torch.nn.functional.pad(t[..., c0:], (0, c1_pad - c1))
    return torch.cat([a, b], -1).reshape(co, kh * kw * (c0_pad + c1_pad)).contiguous()


def pack_conv_up2x(w, cin_pad=None):
    """Phase weights of `nearest x2 upsample + 3x3 / pad 1 conv` (SaspaGemmParams.upsample = 2): [Cout, Cin, 3, 3] ->
    [4, Cout, 4*Cin_pad] float64, phase index py*2+px, K index (dy*2+dx)*Cin_pad + c.  Output pixel (2i+py, 2j+px) sees the
    hi-res rows 2i+py-1 .. 2i+py+1, which fall on the low-res rows {i-1, i, i} (py = 0) or {i, i, i+1} (py = 1): a 2x2
    correlation over the low-res input with its window at (i+py-1, j+px-1), whose taps are the SUMS of the 3x3 taps that share
    a low-res pixel -- rows {0}, {1, 2} for py = 0 and {0, 1}, {2} for py = 1, columns alike.  Summed in float64 from the
    master weights and returned unrounded: the caller rounds ONCE, to the storage type."""
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3), "phase weights exist for the 3x3 window only"
    cp = round8(ci) if cin_pad is None else cin_pad
    t = w.detach().to(torch.float64).permute(0, 2, 3, 1)                 # [Cout, ky, kx, Cin]
    sets = (((0,), (1, 2)), ((0, 1), (2,)))                              # [phase bit][tap of the 2x2 window] -> 3x3 taps
    out = torch.zeros((4, co, 2, 2, cp), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    acc = torch.zeros((co, ci), dtype=torch.float64)
                    for ky in sets[py][dy]:
                        for kx in sets[px][dx]:
                            acc += t[:, ky, kx, :]
                    out[py * 2 + px, :, dy, dx, :ci] = acc
    return out.reshape(4, co, 4 * cp).contiguous()


def ktile(dtype):
    """Elements of one K-tile of the implicit GEMM (128 bytes per row): 64 of the 16-bit compute type (bf16 / fp16) / 32 fp32."""
    return 64 if dtype in (torch.bfloat16, torch.float16) else 32


def chunk_major_ok(kh, kw, c0_pad, c1_pad, dtype):
    """A conv can be packed chunk-major (SASPA_KORDER_CHUNK) when it has a window and its (padded) source channel counts
    are whole K-tiles -- exactly the layers the LDS-DMA kernels run."""
    import os
    if os.environ.get("SASPA_KORDER", "1") == "0":          # A/B knob: keep every conv tap-major
        return False
    bk = ktile(dtype)
    return kh * kw > 1 and c0_pad % bk == 0 and c1_pad % bk == 0


def to_chunk_major(packed, taps, dtype):
    """[N, taps*C] tap-major (K = tap*C + c) -> chunk-major (K = (chunk*taps + tap)*bk + c_in_chunk)."""
    n, k = packed.shape
    bk = ktile(dtype)
    c = k // taps
    assert c * taps == k and c % bk == 0
    return packed.view(n, taps, c // bk, bk).permute(0, 2, 1, 3).reshape(n, k).contiguous()


def pack_ff_block(w1, b1, w2, b2):
    """Operands of `saspa_ff_block` (include/saspa_hip.h) from a GEGLU feed-forward: ff.net.0.proj.weight `w1` [2F, 320] (rows 0..F-1
    values, F..2F-1 gates: diffusers' `hidden, gate = proj(x).chunk(2, -1)`), its bias `b1` [2F], ff.net.2.weight `w2` [320, F] and
    bias `b2` [320] -> (w1p [2F, 320] fp32, b1p [2F] fp32, w2f [F/32, 10, 2, 64, 8] fp32, b2 [320] fp32):
    * w1p / b1p: per slice t of 32 features the 32 value rows followed by their 32 gate rows;
    * w2f: MFMA A-operand fragments of W2 -- fragment (t, nb, s), lane = m + 32 h, element e = W2[32 nb + m][32 t + 16 s + (e & 3) +
      8 (e >> 2) + 4 h]: the K order in which the kernel's GEGLU stage leaves its packed accumulator registers."""
    w1, b1, w2, b2 = w1.float(), b1.float(), w2.float(), b2.float()
    f = w2.shape[1]
    if w1.shape != (2 * f, 320) or w2.shape[0] != 320 or f % 32 or b1.numel() != 2 * f or b2.numel() != 320:
        raise ValueError(f"pack_ff_block: unexpected shapes {tuple(w1.shape)} {tuple(w2.shape)}")
    t = f // 32
    w1p = torch.cat([w1[:f].reshape(t, 32, 320), w1[f:].reshape(t, 32, 320)], 1).reshape(2 * f, 320).contiguous()
    b1p = torch.cat([b1[:f].reshape(t, 32), b1[f:].reshape(t, 32)], 1).reshape(2 * f).contiguous()
    e = torch.arange(8)
    fidx = 16 * torch.arange(2)[:, None, None] + 4 * torch.arange(2)[None, :, None] + ((e & 3) + 8 * (e >> 2))[None, None, :]   # [s, h, e]
    g = w2.reshape(10, 32, t, 32)[:, :, :, fidx]                     # [nb, m, t, s, h, e]
    w2f = g.permute(2, 0, 3, 4, 1, 5).reshape(t, 10, 2, 64, 8).contiguous()
    return w1p, b1p, w2f, b2.contiguous()


def presplit_x3(w):
    """[N, K] fp32 packed weights (any K order, K % 32 == 0) -> the same [N, K] fp32-typed buffer holding, per K-tile of 32 values
    (128 bytes), [32 bf16 hi | 32 bf16 lo] with hi = bf16(w), lo = bf16(w - hi) (round to nearest even, what the SASPA_F32X3 loop
    computes in registers), in the order a lane consumes the tile: 16-byte chunk c of either half = tile positions 4c..4c+3,
    16+4c..16+4c+3 (lane group c reads fp32 chunks c and 4 + c of the ACTIVATION tile).  SaspaGemmParams.w_split (ABI 20): the
    K loop then splits the activations only."""
    n, k = w.shape
    if k % 32 or w.dtype != torch.float32:
        raise ValueError("presplit_x3 wants fp32 [N, K] with K % 32 == 0")
    idx = torch.tensor([q for c in range(4) for q in (list(range(4 * c, 4 * c + 4)) + list(range(16 + 4 * c, 20 + 4 * c)))], device=w.device)
    t = w.reshape(n, k // 32, 32)[:, :, idx]
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    out = torch.cat([hi, lo], dim=2).reshape(n, 2 * k).contiguous().view(torch.float32)
    assert out.shape == (n, k)
    return out


def to_chunk32_major(packed, taps=9):
    """[N, taps*C] tap-major -> K = ((chunk32 * taps + tap) * 32 + c_in_chunk): the packing of saspa_conv3x3_halo
    (SASPA_KORDER_CHUNK32: one (chunk32, tap) slot is one half of a 64-deep K-tile)."""
    n, k = packed.shape
    c = k // taps
    assert c * taps == k and c % 32 == 0
    return packed.view(n, taps, c // 32, 32).permute(0, 2, 1, 3).reshape(n, k).contiguous()


def pack_gamma_beta32(gamma, beta):
    """GroupNorm affine -> [C / 32][64] fp32: per 32-channel chunk gamma[32] | beta[32] (SaspaConvGnParams.gamma_beta32: one
    256-byte LDS-DMA piece per chunk)."""
    c = gamma.numel()
    assert c % 32 == 0 and beta.numel() == c
    return torch.cat([gamma.float().reshape(-1, 32), beta.float().reshape(-1, 32)], 1).contiguous()


def pack_linear(w, k_pad=None):
    n, k = w.shape
    kp = round8(k) if k_pad is None else k_pad
    if kp != k:
        w = torch.nn.functional.pad(w, (0, kp - k))
    return w.contiguous()


def quantize_fp8(w):
    """[N, K] fp32 weight -> (e4m3 bytes as uint8 [N, K], per-output-channel scale fp32 [N]) with w ~ q * scale[:, None]
    (scale = row amax / 448, OCP e4m3fn as the gfx950 MFMA reads it)."""
    w = w.float()
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (w / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def pack_conv_mxfp8(w):
    """[Cout, Cin, 3, 3] fp32 conv weight -> (e4m3 bytes uint8 [Cout, Kp], per-output-channel scale fp32 [Cout]) for
    saspa_conv3x3_mxfp8: K = (ky*3+kx)*Cin + c (pack_conv's tap-major order, no channel padding), zero padded to Kp = a
    multiple of 128; the scales of quantize_fp8 on the packed matrix (the padding is zero, so it changes no row maximum)."""
    pk = pack_conv(w.float(), cin_pad=w.shape[1])
    k = pk.shape[1]
    kp = (k + 127) // 128 * 128
    if kp != k:
        pk = torch.nn.functional.pad(pk, (0, kp - k))
    return quantize_fp8(pk)


def dequantize_fp8(q_u8, scale):
    return q_u8.view(torch.float8_e4m3fn).float() * scale[:, None]


def pack_geglu_tile(w, b, bn):
    """pack_geglu with an explicit tile width (the fp8 kernel's tiles are 128 columns: 64 values then their 64 gates)."""
    n = w.shape[0]
    f = n // 2
    if n % bn:
        return None
    half = bn // 2
    idx = []
    for t in range(n // bn):
        idx += list(range(t * half, (t + 1) * half)) + list(range(f + t * half, f + (t + 1) * half))
    idx = torch.tensor(idx)
    return w[idx].contiguous(), b[idx].contiguous()


def geglu_tile(n):
    """Output-tile width the GEMM picks for N columns (must mirror csrc/saspa_gemm.hip)."""
    return 160 if n % 160 == 0 else 128


def pack_geglu(w, b):
    """GEGLU.proj weight [2F, K] / bias [2F] -> rows regrouped per output tile so the fused
    epilogue finds each feature's value and gate in the same tile: tile t = [values of features
    t*BN/2 .. (t+1)*BN/2), then their gates].  Returns None when 2F is not a whole number of tiles."""
    n = w.shape[0]
    f = n // 2
    bn = geglu_tile(n)
    if n % bn:
        return None
    half = bn // 2
    idx = []
    for t in range(n // bn):
        idx += list(range(t * half, (t + 1) * half)) + list(range(f + t * half, f + (t + 1) * half))
    idx = torch.tensor(idx)
    return w[idx].contiguous(), b[idx].contiguous()


# ---- fused cross-attention block (csrc/saspa_xattn.hip, include/saspa_hip.h: SaspaXattnBlockParams) -------------------------
XATTN_C, XATTN_HEADS, XATTN_D = 320, 8, 40


def _xattn_rho(pos):
    """Row (0..15) of a 16-deep MFMA K-step that operand position `pos` = 8 * (lane half) + element j holds when the operand is
    an accumulator tile packed to bf16 (v_mfma_f32_32x32x16_bf16: register r of lane half h is row (r & 3) + 8 (r >> 2) + 4 h)."""
    h, j = pos >> 3, pos & 7
    return 8 * (j >> 2) + 4 * h + (j & 3)


def pack_xattn_w(wq, wo, bo):
    """to_q [320, 320] (softmax scale * log2 e already folded in), to_out [320, 320], to_out bias [320] (fp32, host) -> the stacked
    [640, 320] matrix and the [640] bias saspa_xattn_block streams:
      rows 0..319   to_q rows ordered [head 0..7: channels 0..31 | head 0..7: channels 32..39] -- a head is one whole 32-row
                    accumulator block plus a quarter of a tail block;
      rows 320..639 to_out with its K columns in the order the attention stage emits O^T: K-step ks < 16 = channels 16 (ks & 1)
                    + rho of head ks >> 1, K-steps 16..19 = the channel-32..39 tails of heads (2 i, 2 i + 1), inside every K-step
                    the operand positions follow `_xattn_rho`."""
    d, c = XATTN_D, XATTN_C
    assert tuple(wq.shape) == (c, c) and tuple(wo.shape) == (c, c) and bo.numel() == c
    rows = [b * d + i for b in range(XATTN_HEADS) for i in range(32)] + [(t // 8) * d + 32 + (t % 8) for t in range(64)]
    feat = []
    for ks in range(c // 16):
        for pos in range(16):
            rho = _xattn_rho(pos)
            if ks < 16:
                feat.append((ks >> 1) * d + 16 * (ks & 1) + rho)
            else:
                feat.append((2 * (ks - 16) + (rho >> 3)) * d + 32 + (rho & 7))
    assert sorted(rows) == list(range(c)) and sorted(feat) == list(range(c))
    w = torch.cat([wq.float()[torch.tensor(rows)], wo.float()[:, torch.tensor(feat)]], 0).contiguous()
    bias = torch.cat([torch.zeros(c), bo.float().reshape(-1)]).contiguous()
    return w, bias


_XATTN_IDX = {}


def _xattn_frag_indices(device):
    """Gather indices into a per-head [96 keys][48 channel slots] plane for the K fragments [3][3][64][8] and the V^T fragments
    [2][6][64][8] of saspa_xattn_block (slot 47 is always zero: the 'nothing here' target)."""
    key = str(device)
    if key in _XATTN_IDX:
        return _XATTN_IDX[key]
    kf = torch.zeros((3, 3, 64, 8), dtype=torch.long)
    vf = torch.zeros((2, 6, 64, 8), dtype=torch.long)
    for lane in range(64):
        m, h = lane & 31, lane >> 5
        for j in range(8):
            rho = 8 * (j >> 2) + 4 * h + (j & 3)
            for kb in range(3):
                k = 32 * kb + m
                for s_ in range(3):
                    if s_ < 2:
                        dd = 16 * s_ + rho
                    else:
                        dd = 32 + 4 * h + (j & 3) if j < 4 else 47
                    kf[kb, s_, lane, j] = k * 48 + dd
            for db in range(2):
                dd = 32 * db + m
                for ks in range(6):
                    k = 16 * ks + rho
                    vf[db, ks, lane, j] = k * 48 + (dd if dd < 47 else 47)
    _XATTN_IDX[key] = (kf.reshape(-1).to(device), vf.reshape(-1).to(device))
    return _XATTN_IDX[key]


def xattn_kv_fragments(k, v):
    """Text keys / values of one transformer block, k and v [B, nk, 320] (device, bf16, nk <= 96), -> (kf [B, 8 * 9 * 64 * 8],
    vf [B, 8 * 12 * 64 * 8]) bf16: the MFMA A-operand fragments saspa_xattn_block loads (layouts in include/saspa_hip.h).
    Time-invariant: built once per generation next to the K / V projections themselves."""
    b, nk, c = k.shape
    assert c == XATTN_C and nk <= 96 and tuple(v.shape) == (b, nk, c)
    ik, iv = _xattn_frag_indices(k.device)
    kp = torch.zeros((b, XATTN_HEADS, 96, 48), device=k.device, dtype=k.dtype)
    kp[:, :, :nk, :XATTN_D] = k.reshape(b, nk, XATTN_HEADS, XATTN_D).permute(0, 2, 1, 3)
    vp = torch.zeros((b, XATTN_HEADS, 96, 48), device=k.device, dtype=k.dtype)
    vp[:, :, :nk, :XATTN_D] = v.reshape(b, nk, XATTN_HEADS, XATTN_D).permute(0, 2, 1, 3)
    vp[:, :, :nk, XATTN_D] = 1.0                           # the ones row: the softmax denominator out of the P V product
    kf = kp.reshape(b, XATTN_HEADS, 96 * 48)[:, :, ik].reshape(b, -1).contiguous()
    vf = vp.reshape(b, XATTN_HEADS, 96 * 48)[:, :, iv].reshape(b, -1).contiguous()
    return kf, vf
