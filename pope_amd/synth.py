"""Seeded synthetic inputs and weights for the hot path.

Real checkpoints (weights/dinov2_vits14.pth, weights/matcher.pth) cannot be
fetched offline, so benchmarks, smoke and parity tests use
seeded synthetic weights in the reference's exact state-dict layout
(dinov2/dinov2/models/vision_transformer.py:45-163 -> 175 keys for ViT-S/14).
"""
import math

import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)  # segment_anything/segment_anything/dinov2_utils.py:67
IMAGENET_STD = (0.229, 0.224, 0.225)


def synthetic_state_dict(seed=0, dim=384, depth=12, patch=14, grid=37, gamma=1.0,
                         wscale=None, ffn="mlp"):
    """Seeded synthetic weights in the reference checkpoint layout (175 keys for
    ViT-S/14).  Unlike the reference initialisers (gamma=1e-5,
    trunc_normal(0.02)), branch outputs here are O(1) so that attention / MLP
    kernels are actually exercised."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float32) * std

    sd = {}
    sd["cls_token"] = rn(1, 1, dim, std=0.5)
    sd["pos_embed"] = rn(1, grid * grid + 1, dim, std=0.2)
    sd["mask_token"] = torch.zeros(1, dim)
    k_pe = 3 * patch * patch
    sd["patch_embed.proj.weight"] = rn(dim, 3, patch, patch, std=1.0 / math.sqrt(k_pe))
    sd["patch_embed.proj.bias"] = rn(dim, std=0.1)
    ws = wscale if wscale is not None else 1.0
    for i in range(depth):
        p = f"blocks.{i}."
        sd[p + "norm1.weight"] = 1.0 + rn(dim, std=0.1)
        sd[p + "norm1.bias"] = rn(dim, std=0.05)
        sd[p + "attn.qkv.weight"] = rn(3 * dim, dim, std=ws * 1.5 / math.sqrt(dim))
        sd[p + "attn.qkv.bias"] = rn(3 * dim, std=0.1)
        sd[p + "attn.proj.weight"] = rn(dim, dim, std=ws / math.sqrt(dim))
        sd[p + "attn.proj.bias"] = rn(dim, std=0.05)
        sd[p + "ls1.gamma"] = gamma * (0.3 + 0.1 * rn(dim))
        sd[p + "norm2.weight"] = 1.0 + rn(dim, std=0.1)
        sd[p + "norm2.bias"] = rn(dim, std=0.05)
        if ffn == "swiglu":   # SwiGLUFFNFused (swiglu_ffn.py:45-63): w12 [2 h, dim], w3 [dim, h], same O(1) recipe
            h = (int(4 * dim * 2 / 3) + 7) // 8 * 8
            sd[p + "mlp.w12.weight"] = rn(2 * h, dim, std=ws / math.sqrt(dim))
            sd[p + "mlp.w12.bias"] = rn(2 * h, std=0.1)
            sd[p + "mlp.w3.weight"] = rn(dim, h, std=ws / math.sqrt(h))
            sd[p + "mlp.w3.bias"] = rn(dim, std=0.05)
        else:
            sd[p + "mlp.fc1.weight"] = rn(4 * dim, dim, std=ws / math.sqrt(dim))
            sd[p + "mlp.fc1.bias"] = rn(4 * dim, std=0.1)
            sd[p + "mlp.fc2.weight"] = rn(dim, 4 * dim, std=ws / math.sqrt(4 * dim))
            sd[p + "mlp.fc2.bias"] = rn(dim, std=0.05)
        sd[p + "ls2.gamma"] = gamma * (0.3 + 0.1 * rn(dim))
    sd["norm.weight"] = 1.0 + rn(dim, std=0.1)
    sd["norm.bias"] = rn(dim, std=0.05)
    return sd


def synthetic_sam_encoder_state_dict(seed=0, dim=1280, depth=32, heads=16, grid=64, window=14, global_idx=(7, 15, 23, 31),
                                     patch=16, out_chans=256):
    """Seeded synthetic weights in the layout of SAM's `ImageEncoderViT` state dict
    (segment_anything/segment_anything/modeling/image_encoder.py:53-105, build_sam.py:66-79; ViT-H defaults).  Branch
    outputs and the relative-position terms are O(1) so windows, padding keys and the bias all matter."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float32) * std

    hd = dim // heads
    sd = {"pos_embed": rn(1, grid, grid, dim, std=0.2)}
    k_pe = 3 * patch * patch
    sd["patch_embed.proj.weight"] = rn(dim, 3, patch, patch, std=1.0 / math.sqrt(k_pe))
    sd["patch_embed.proj.bias"] = rn(dim, std=0.1)
    for i in range(depth):
        p = f"blocks.{i}."
        size = grid if i in global_idx else window
        sd[p + "norm1.weight"] = 1.0 + rn(dim, std=0.1)
        sd[p + "norm1.bias"] = rn(dim, std=0.05)
        sd[p + "attn.qkv.weight"] = rn(3 * dim, dim, std=1.5 / math.sqrt(dim))
        sd[p + "attn.qkv.bias"] = rn(3 * dim, std=0.1)
        sd[p + "attn.proj.weight"] = rn(dim, dim, std=0.3 / math.sqrt(dim))
        sd[p + "attn.proj.bias"] = rn(dim, std=0.02)
        sd[p + "attn.rel_pos_h"] = rn(2 * size - 1, hd, std=0.15)
        sd[p + "attn.rel_pos_w"] = rn(2 * size - 1, hd, std=0.15)
        sd[p + "norm2.weight"] = 1.0 + rn(dim, std=0.1)
        sd[p + "norm2.bias"] = rn(dim, std=0.05)
        sd[p + "mlp.lin1.weight"] = rn(4 * dim, dim, std=1.0 / math.sqrt(dim))
        sd[p + "mlp.lin1.bias"] = rn(4 * dim, std=0.1)
        sd[p + "mlp.lin2.weight"] = rn(dim, 4 * dim, std=0.3 / math.sqrt(4 * dim))
        sd[p + "mlp.lin2.bias"] = rn(dim, std=0.02)
    sd["neck.0.weight"] = rn(out_chans, dim, 1, 1, std=1.0 / math.sqrt(dim))
    sd["neck.1.weight"] = 1.0 + rn(out_chans, std=0.1)
    sd["neck.1.bias"] = rn(out_chans, std=0.05)
    sd["neck.2.weight"] = rn(out_chans, out_chans, 3, 3, std=1.0 / math.sqrt(9 * out_chans))
    sd["neck.3.weight"] = 1.0 + rn(out_chans, std=0.1)
    sd["neck.3.bias"] = rn(out_chans, std=0.05)
    return sd


def synthetic_images(batch, h=476, w=630, seed=0, device="cpu"):
    """Uniform[0,1) 640x480 frames, centre-cropped to (h, w) and normalised with
    the ImageNet statistics of set_torch_image."""
    g = torch.Generator().manual_seed(seed)
    full_h, full_w = max(480, h), max(640, w)
    img = torch.rand(batch, 3, full_h, full_w, generator=g, dtype=torch.float32)
    top, left = (full_h - h) // 2, (full_w - w) // 2
    img = img[:, :, top:top + h, left:left + w]
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    return ((img - mean) / std).contiguous().to(device)


def synthetic_pairs(n_pairs, h=476, w=630, seed=0, shift=(14, 28), noise=0.1, device="cpu"):
    """Pair = (img, roll(img, shift) + N(0, noise^2)) so the dense matcher emits
    ~ (H/14-4-1)*(W/14-4-2) matches per pair instead of none."""
    img0 = synthetic_images(n_pairs, h, w, seed, "cpu")
    g = torch.Generator().manual_seed(seed + 7919)
    img1 = torch.roll(img0, shifts=shift, dims=(2, 3))
    if noise > 0:
        img1 = img1 + noise * torch.randn(img1.shape, generator=g, dtype=torch.float32)
    return img0.to(device), img1.contiguous().to(device)


def _hash_uniform(ids, n_per, salt, device):
    """[len(ids), n_per] floats in [0, 1): a counter-based integer hash of (id, element index, salt).  Integer and
    exact-float arithmetic only, so a pair's pixels depend on its id alone — not on the batch it rides in, the rank
    that owns it or the device that evaluates the expression."""
    i = torch.arange(n_per, device=device, dtype=torch.int64)[None, :]
    x = (ids.to(device=device, dtype=torch.int64)[:, None] * 0x9E3779B1 + i * 0x85EBCA6B + salt * 0xC2B2AE35) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 0x846CA68B) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    return (x >> 8).to(torch.float32) / 16777216.0


def pairs_by_id(ids, h=476, w=630, shift=(14, 28), noise=0.1, device="cpu"):
    """Synthetic pixels for the pairs of a work list (BASELINE config 4: only the pair ids of the LINEMOD list
    travel): frame = hash-uniform 640x480, centre crop (h, w), ImageNet normalisation; the second image
    is the rolled first plus noise * (Irwin-Hall sum of four hash-uniforms, unit variance)."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    n, full_h, full_w = len(ids), max(480, h), max(640, w)
    img = _hash_uniform(ids, 3 * full_h * full_w, 1, device).view(n, 3, full_h, full_w)
    top, left = (full_h - h) // 2, (full_w - w) // 2
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    img0 = ((img[:, :, top:top + h, left:left + w] - mean) / std).contiguous()
    del img
    img1 = torch.roll(img0, shifts=shift, dims=(2, 3))
    if noise > 0:
        z = sum(_hash_uniform(ids, 3 * h * w, 2 + k, device) for k in range(4)).view(n, 3, h, w)
        img1 = img1 + (noise * math.sqrt(3.0)) * (z - 2.0)
    return img0, img1.contiguous()


def synthetic_matcher_state_dict(seed=0, cfg=None):
    """Seeded synthetic LoFTR `Matcher` weights in the reference checkpoint layout (211 keys,
    src/matcher/matcher.py:18-27; weights/matcher.pth is not available offline).  Fan-in scaled normal
    filters; BatchNorm statistics and affines are randomised (the reference's fresh-module defaults are
    the identity, which would not exercise BN folding)."""
    if cfg is None:
        from .matcher import default_cfg as cfg
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float32) * std

    def ru(*shape, lo=0.5, hi=1.5):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float32)

    sd = {}

    def conv(name, cout, cin, k, gain=1.0):
        sd[name + ".weight"] = rn(cout, cin, k, k, std=math.sqrt(gain / (cin * k * k)))

    def bn(name, c):
        sd[name + ".weight"] = ru(c)
        sd[name + ".bias"] = rn(c, std=0.1)
        sd[name + ".running_mean"] = rn(c, std=0.1)
        sd[name + ".running_var"] = ru(c)
        sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)

    d0 = cfg["resnetfpn"]["initial_dim"]
    d1, d2, d3 = cfg["resnetfpn"]["block_dims"]
    conv("backbone.conv1", d0, 1, 7, gain=8.0)
    bn("backbone.bn1", d0)
    cin = d0
    for li, (dim, stride) in enumerate(((d1, 1), (d2, 2), (d3, 2)), start=1):
        for bi in range(2):
            p = f"backbone.layer{li}.{bi}"
            conv(p + ".conv1", dim, cin if bi == 0 else dim, 3)
            conv(p + ".conv2", dim, dim, 3)
            bn(p + ".bn1", dim)
            bn(p + ".bn2", dim)
            if bi == 0 and stride != 1:
                conv(p + ".downsample.0", dim, cin, 1)
                bn(p + ".downsample.1", dim)
        cin = dim
    conv("backbone.layer3_outconv", d3, d3, 1, gain=2.0)
    conv("backbone.layer2_outconv", d3, d2, 1)
    conv("backbone.layer2_outconv2.0", d3, d3, 3)
    bn("backbone.layer2_outconv2.1", d3)
    conv("backbone.layer2_outconv2.3", d2, d3, 3)
    conv("backbone.layer1_outconv", d2, d1, 1)
    conv("backbone.layer1_outconv2.0", d2, d2, 3)
    bn("backbone.layer1_outconv2.1", d2)
    conv("backbone.layer1_outconv2.3", d1, d2, 3)

    def transformer(prefix, c):
        # small LayerNorm gains keep the residual stream O(1): with unit gains eight layers of O(1) messages
        # make <f0,f1>/(C*0.1) so large that the dual softmax saturates to exact 0/1 confidences
        d, n_layers = c["d_model"], len(c["layer_names"])
        for i in range(n_layers):
            p = f"{prefix}.layers.{i}."
            for nm in ("q_proj", "k_proj", "v_proj", "merge"):
                sd[p + nm + ".weight"] = rn(d, d, std=1.0 / math.sqrt(d))
            sd[p + "mlp.0.weight"] = rn(2 * d, 2 * d, std=1.0 / math.sqrt(2 * d))
            sd[p + "mlp.2.weight"] = rn(d, 2 * d, std=math.sqrt(2.0 / (2 * d)))
            for nm in ("norm1", "norm2"):
                sd[p + nm + ".weight"] = ru(d, lo=0.3, hi=0.5)
                sd[p + nm + ".bias"] = rn(d, std=0.02)

    transformer("loftr_coarse", cfg["coarse"])
    dc, df = cfg["coarse"]["d_model"], cfg["fine"]["d_model"]
    sd["fine_preprocess.down_proj.weight"] = rn(df, dc, std=1.0 / math.sqrt(dc))
    sd["fine_preprocess.down_proj.bias"] = rn(df, std=0.05)
    sd["fine_preprocess.merge_feat.weight"] = rn(df, 2 * df, std=1.0 / math.sqrt(2 * df))
    sd["fine_preprocess.merge_feat.bias"] = rn(df, std=0.05)
    transformer("loftr_fine", cfg["fine"])
    return sd


def peaked_matcher_state_dict(pre_outconv, seed=0, gain=2.0, cfg=None):
    """Synthetic LoFTR weights under which the `Matcher` behaves like a trained one on related image pairs: hundreds of
    confident matches per 256 x 256 pair (the interior maximum of (32 - 4)^2 cells minus the shifted border), instead of the
    handful the plain random weights give.  Why those give so few: the 1/8-resolution features are f_i = v + d_i with a
    common vector v (the mean of the post-ReLU activations through the bias-free 1x1 output convolution, |v|^2 = 1 400) that
    swamps the cell-specific part (|d|^2 = 180): <v, d_j> acts as a per-column bias in the dual softmax and one column
    attracts every row.  A trained network has no such component.  Here it is projected out: W' = gain * W (I - m m^T / |m|^2)
    with m the mean of the activations in front of `backbone.layer3_outconv` on a calibration batch of the same image
    statistics (`synthetic_gray_pairs`), which leaves features whose correlation picks the true cell for 3 of 4 cells before
    the transformer and whose dual-softmax confidence clears 0.9 on 95 % of the interior cells.
    `pre_outconv(state_dict, images[n, 1, H, W]) -> activations [n, 256, H / 8, W / 8]` runs the CNN up to that convolution
    (pass a state dict whose `backbone.layer3_outconv.weight` is the identity to any implementation of the backbone: the HIP
    module — `hip_pre_outconv` below — on the GPU box, the CPU checker in the CPU tests); this module computes nothing itself.
    `pre_outconv` may also be the calibration mean m itself ([256] tensor, e.g. from a fixture).  The returned dict carries it
    under "_calibration_mean" — pop it before `load_state_dict`."""
    sd = synthetic_matcher_state_dict(seed, cfg)
    w = sd["backbone.layer3_outconv.weight"]
    c = w.shape[0]
    if torch.is_tensor(pre_outconv):   # the calibration mean itself (a fixture pins the weights bit for bit across hosts)
        m = pre_outconv.detach().double().cpu().reshape(c)
    else:
        ident = dict(sd)
        ident["backbone.layer3_outconv.weight"] = torch.eye(c).reshape(c, c, 1, 1)
        cal = synthetic_gray_pairs(4, 256, 256, seed=1000 + seed)[0]
        x3 = pre_outconv(ident, cal).detach().float().cpu()
        m = x3.permute(0, 2, 3, 1).reshape(-1, c).double().mean(0)
    sd["_calibration_mean"] = m.clone()    # not a checkpoint key: callers that need it pop it (load_state_dict would reject it)
    mh = m / m.norm()
    proj = torch.eye(c, dtype=torch.float64) - torch.outer(mh, mh)
    sd["backbone.layer3_outconv.weight"] = (gain * (w.reshape(c, c).double() @ proj)).float().reshape(c, c, 1, 1).contiguous()
    return sd


def hip_pre_outconv(device):
    """`pre_outconv` of `peaked_matcher_state_dict` on the HIP backbone (pope_amd/loftr.py:ResNetFPN_8_2)."""
    def run(sd, images):
        from .loftr import build_backbone
        from .matcher import default_cfg
        bb = build_backbone(default_cfg).eval()
        bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
        return bb.to(device)(images.to(device))[0]
    return run


def synthetic_gray_pairs(n_pairs, h=256, w=256, seed=0, shift=(8, 16), noise=0.02):
    """Grayscale [n,1,h,w] pairs in [0,1] for the LoFTR `Matcher` (the drivers feed 256x256 crops,
    eval_linemod_json.py:103-111): image1 = roll(image0, shift) + noise, h and w multiples of 8."""
    g = torch.Generator().manual_seed(seed)
    # low-pass random texture: LoFTR's CNN sees structure rather than white noise
    base = torch.rand(n_pairs, 1, h // 4, w // 4, generator=g, dtype=torch.float32)
    img0 = torch.nn.functional.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)
    img0 = (0.7 * img0 + 0.3 * torch.rand(n_pairs, 1, h, w, generator=g, dtype=torch.float32)).clamp_(0, 1)
    img1 = torch.roll(img0, shifts=shift, dims=(2, 3))
    if noise > 0:
        img1 = (img1 + noise * torch.randn(img1.shape, generator=g, dtype=torch.float32)).clamp_(0, 1)
    return img0.contiguous(), img1.contiguous()


def synthetic_driver_case(n_proposals=8, seed=31):
    """Synthetic stand-in for one iteration of the drivers' pair loop (eval_linemod_json.py:52-127) without
    SAM / cv2: a reference crop, P proposal crops for DINOv2 (196x196, the drivers' centre-crop size) and the
    matching gray images for LoFTR (256x256).  Proposals 2, 5 and 6 show the reference object (shifted,
    increasingly noisy), proposal 3 duplicates proposal 2's DINOv2 crop exactly (a score tie), the others
    are unrelated texture."""
    g = torch.Generator().manual_seed(seed)
    ref_tensor = synthetic_images(1, 196, 196, seed=seed)
    crop_tensors = synthetic_images(n_proposals, 196, 196, seed=seed + 1)
    gray_ref = synthetic_gray_pairs(1, 256, 256, seed=seed)[0]
    gray_crops = synthetic_gray_pairs(n_proposals, 256, 256, seed=seed + 2)[0]
    for p, (noise_rgb, shift, noise_gray) in {2: (0.3, (8, 16), 0.01), 5: (0.6, (16, 8), 0.03),
                                              6: (1.0, (24, 24), 0.06)}.items():
        crop_tensors[p] = ref_tensor[0] + noise_rgb * torch.randn(ref_tensor[0].shape, generator=g)
        gray_crops[p] = (torch.roll(gray_ref[0], shifts=shift, dims=(1, 2))
                         + noise_gray * torch.randn(gray_ref[0].shape, generator=g)).clamp_(0, 1)
    crop_tensors[3] = crop_tensors[2]
    return ref_tensor, crop_tensors, gray_ref, gray_crops


def synthetic_pose_scene(n, seed, outlier=0.3, noise=0.0, K0=None, K1=None):
    """A planted two-view scene for the pose solver: n 3-D points in front of both cameras, a random
    rotation of 5-30 degrees and a unit-direction translation of length 0.5, projected with K0 / K1 (defaults: the LINEMOD
    camera and a 256x256 crop camera, the two intrinsics eval_linemod_json.py:160 passes), Gaussian pixel noise, and a
    fraction `outlier` of the second image's points replaced by uniform clutter.
    Returns numpy (kpts0 [n,2] f32, kpts1 [n,2] f32, K0, K1, R [3,3], t [3], planted_inlier [n] bool)."""
    import numpy as np
    g = np.random.default_rng(seed)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(g.uniform(5, 30))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = g.normal(size=3)
    t *= 0.5 / np.linalg.norm(t)
    X = np.stack([g.uniform(-1, 1, n), g.uniform(-1, 1, n), g.uniform(3, 6, n)], 1)
    K0 = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]]) if K0 is None else np.asarray(K0, np.float64)
    K1 = np.array([[600.0, 0, 128.0], [0, 610.0, 120.0], [0, 0, 1.0]]) if K1 is None else np.asarray(K1, np.float64)
    p0 = (X / X[:, 2:]) @ K0.T
    X1 = X @ R.T + t
    p1 = (X1 / X1[:, 2:]) @ K1.T
    k0 = p0[:, :2] + g.normal(size=(n, 2)) * noise
    k1 = p1[:, :2] + g.normal(size=(n, 2)) * noise
    n_out = int(outlier * n)
    bad = g.permutation(n)[:n_out]
    k1[bad] = np.stack([g.uniform(0, 256, n_out), g.uniform(0, 256, n_out)], 1)
    inl = np.ones(n, bool)
    inl[bad] = False
    return k0.astype(np.float32), k1.astype(np.float32), K0, K1, R, t, inl


def synthetic_frame_case(n_proposals=8, seed=31, frame_hw=(480, 640)):
    """uint8 stand-in for one query of the drivers' loop starting at the raw frame (eval_linemod_json.py:62-90), without SAM:
    a 256x256 BGR reference crop, a BGR frame and P proposal boxes (x, y, w, h).  Proposals 1 and 4 are 160x160 boxes whose
    30 %-expanded window (256x256, scale 1: an integer crop) shows the reference shifted by a few pixels plus noise, so the
    DINOv2 vote and the LoFTR matcher (synthetic weights) find them; the other boxes of assorted sizes — two leave the frame —
    sit on unrelated texture.  Returns numpy (ref_bgr [256,256,3], frame_bgr [H,W,3], bboxes_xywh [P,4], K0 [3,3], K1 [3,3])."""
    import numpy as np
    H, W = frame_hw
    g = torch.Generator().manual_seed(seed)

    def texture(h, w):
        base = torch.rand(1, 3, h // 4 + 1, w // 4 + 1, generator=g)
        t = torch.nn.functional.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)[0]
        return (0.7 * t + 0.3 * torch.rand(3, h, w, generator=g)).clamp_(0, 1)

    ref = texture(256, 256)
    frame = texture(H, W)
    boxes = np.zeros((n_proposals, 4), np.int64)
    planted = {1: ((96, 88), (8, 16), 0.01), 4: ((372, 60), (16, 8), 0.03)}      # (x, y) of the 160-box, shift, noise
    rng = np.random.default_rng(seed)
    for p in range(n_proposals):
        if p in planted:
            (x, y), shift, noise = planted[p]
            win = (torch.roll(ref, shifts=shift, dims=(1, 2)) + noise * torch.randn(ref.shape, generator=g)).clamp_(0, 1)
            frame[:, y - 48:y + 208, x - 48:x + 208] = win
            boxes[p] = (x, y, 160, 160)
        else:
            w, h = int(rng.integers(40, 220)), int(rng.integers(40, 200))
            boxes[p] = (int(rng.integers(-10, W - w + 30)), int(rng.integers(-10, H - h + 30)), w, h)
    if n_proposals > 6:
        boxes[6] = (W - 90, H - 70, 120, 100)       # leaves the frame at the bottom right
    to_u8 = lambda t: (t.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()  # noqa: E731
    K0 = np.array([[572.4114, 0, 128.0], [0, 573.57043, 128.0], [0, 0, 1.0]])
    K1 = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])
    return to_u8(ref), to_u8(frame), boxes, K0, K1


# ---- padded batches for the LoFTR matcher (mask0 / mask1, scale0 / scale1; tests/golden/*masked*.npz) ----------------------
MASKED_LOFTR_CASES = ("loftr_masked_256", "loftr_masked_192x256_vs_256x192")


def masked_loftr_case(name):
    """Inputs of a padded Matcher batch: dict(image0, image1, mask0, mask1, scale0, scale1) on the CPU plus `thr`.
    loftr_masked_256: the images of loftr_256_lowthr; pair 0 has image0 rows >= 192 and image1 columns >= 200 zeroed, with
    coarse masks off from row 24 / column 25; pair 1 carries all-ones masks.  loftr_masked_192x256_vs_256x192: the images of
    loftr_192x256_vs_256x192 (one pair, different shapes), image0 columns >= 224 and image1 rows >= 216 zeroed (masks off from
    coarse column 28 / row 27)."""
    if name == "loftr_masked_256":
        i0, i1 = synthetic_gray_pairs(2, 256, 256, seed=21)
        m0 = torch.ones(2, 32, 32, dtype=torch.bool)
        m1 = torch.ones(2, 32, 32, dtype=torch.bool)
        i0[0, :, 192:] = 0
        m0[0, 24:] = False
        i1[0, :, :, 200:] = 0
        m1[0, :, 25:] = False
        s0 = torch.tensor([[1.5, 1.25], [0.7, 2.0]])
        s1 = torch.tensor([[1.0, 0.5], [2.0, 1.3]])
    elif name == "loftr_masked_192x256_vs_256x192":
        i0, _ = synthetic_gray_pairs(1, 192, 256, seed=21)
        i1 = synthetic_gray_pairs(1, 256, 192, seed=22)[0]
        i1[:, :, 32:224, :] = i0[:, :, :, 32:224]
        m0 = torch.ones(1, 24, 32, dtype=torch.bool)
        m1 = torch.ones(1, 32, 24, dtype=torch.bool)
        i0[:, :, :, 224:] = 0
        m0[:, :, 28:] = False
        i1[:, :, 216:] = 0
        m1[:, 27:] = False
        s0 = torch.tensor([[1.25, 0.8]])
        s1 = torch.tensor([[0.9, 1.1]])
    else:
        raise KeyError(name)
    return {"image0": i0.contiguous(), "image1": i1.contiguous(), "mask0": m0, "mask1": m1, "scale0": s0, "scale1": s1}, 1e-3


def masked_coarse_case():
    """CoarseMatching inputs (3 pairs on a 12 x 12 grid, C = 256): feat1 = a fixed permutation of feat0 plus noise, so the
    true pairs stand out; pair 0 padded on both sides (rows >= 9 of image 0, columns >= 10 of image 1), pair 1 with a valid
    extent of 4 rows in image 0 (<= 2 * border: no matches), pair 2 with image 1 fully padded.  Returns (feat0, feat1,
    mask0 [3,12,12], mask1 [3,12,12], scale0 [3,2], scale1 [3,2], thr)."""
    g = torch.Generator().manual_seed(5)
    n, h, w, c = 3, 12, 12, 256
    f0 = torch.randn(n, h * w, c, generator=g)
    perm = torch.randperm(h * w, generator=g)
    f1 = f0[:, perm] + 0.3 * torch.randn(n, h * w, c, generator=g)
    m0 = torch.ones(n, h, w, dtype=torch.bool)
    m1 = torch.ones(n, h, w, dtype=torch.bool)
    m0[0, 9:] = False
    m1[0, :, 10:] = False
    m0[1, 4:] = False
    m1[2] = False
    s0 = torch.tensor([[1.5, 0.75], [1.0, 1.0], [0.3, 2.5]])
    s1 = torch.tensor([[0.6, 1.7], [2.0, 0.5], [1.0, 1.0]])
    return f0.contiguous(), f1.contiguous(), m0, m1, s0, s1, 0.2


def masked_coarse_case_large():
    """CoarseMatching inputs at the LoFTR 256 x 256 grid (2 pairs, 32 x 32, C = 256), built like masked_coarse_case, with the
    masks and scales of loftr_masked_256 (pair 0 padded from row 24 of image 0 and column 25 of image 1, pair 1 all ones).
    Returns (feat0, feat1, mask0 [2,32,32], mask1 [2,32,32], scale0 [2,2], scale1 [2,2], thr)."""
    g = torch.Generator().manual_seed(6)
    n, h, w, c = 2, 32, 32, 256
    f0 = torch.randn(n, h * w, c, generator=g)
    perm = torch.randperm(h * w, generator=g)
    f1 = f0[:, perm] + 0.3 * torch.randn(n, h * w, c, generator=g)
    inp, _ = masked_loftr_case("loftr_masked_256")
    return f0.contiguous(), f1.contiguous(), inp["mask0"], inp["mask1"], inp["scale0"], inp["scale1"], 0.2


def masked_xfmr_case():
    """LocalFeatureTransformer inputs with L != S: feat0 [2, 1024, 256] (32 x 32 grid), feat1 [2, 768, 256] (24 x 32) and
    two-sided masks mask0 [2, 1024], mask1 [2, 768] (pair 0 padded in both, pair 1 in image 0 only)."""
    g = torch.Generator().manual_seed(9)
    f0 = torch.randn(2, 1024, 256, generator=g)
    f1 = torch.randn(2, 768, 256, generator=g)
    m0 = torch.ones(2, 32, 32, dtype=torch.bool)
    m1 = torch.ones(2, 24, 32, dtype=torch.bool)
    m0[0, 24:] = False
    m0[1, :, 20:] = False
    m1[0, :, 28:] = False
    return f0, f1, m0.flatten(1), m1.flatten(1)


# ---- Sinkhorn coarse matching (match_type='sinkhorn'; tests/golden/sinkhorn.npz) --------------------------------------------
# name: (pairs, grid 0, grid 1, seed).  "masked_16x16" also carries padding masks and scales; "unrelated" has nothing planted.
SINKHORN_CASES = {
    # L = 192, S = 140: L != S, neither a multiple of a tile.  (Seed searched: under every SINKHORN_SETTINGS entry each row's and
    # column's dustbin stays > 1e-3 relative away from its best real entry; a typical seed leaves ~1e-4 over the ~4000 decisions.)
    "12x16_vs_10x14": (2, (12, 16), (10, 14), 123),
    "32x32": (3, (32, 32), (32, 32), 42),              # the drivers' grid
    "16x16_vs_12x16": (1, (16, 16), (12, 16), 43),
    "masked_16x16": (2, (16, 16), (16, 16), 44),
    "unrelated": (2, (12, 16), (10, 14), 45),
}
# (skh_iters, bin_score, skh_prefilter) run on "12x16_vs_10x14" beside the default (3, 1.0, True)
SINKHORN_SETTINGS = [(it, b, pre) for it in (1, 3) for b in (1.0, 2.5, -0.5) for pre in (True, False)]


def sinkhorn_case(name):
    """CoarseMatching inputs for the Sinkhorn matcher, C = 256: dict(feat0 [n, L, C], feat1 [n, S, C], hw0, hw1, hw0_i) and,
    for "masked_16x16", mask0 / mask1 [n, h, w] bool and scale0 / scale1 [n, 2].  Both sides are N(0, 1); 60 % (masked: 90 %) of the cells of
    the smaller side (of its valid cells, under masks) are copied across under a random permutation with noise 0.3 (a true pair
    then scores ~12 in sim, an unrelated one ~N(0, 0.75)), and everything is scaled by sqrt(12).  "masked_16x16": pair 0 unpadded, pair 1 padded to the
    valid extents 12 x 10 (image 0) and 14 x 16 (image 1)."""
    n, hw0, hw1, seed = SINKHORN_CASES[name]
    g = torch.Generator().manual_seed(seed)
    L, S, c = hw0[0] * hw0[1], hw1[0] * hw1[1], 256
    f0 = torch.randn(n, L, c, generator=g)
    f1 = torch.randn(n, S, c, generator=g)
    m0 = torch.ones(n, *hw0, dtype=torch.bool)
    m1 = torch.ones(n, *hw1, dtype=torch.bool)
    if name == "masked_16x16":
        m0[1, 12:] = False
        m0[1, :, 10:] = False
        m1[1, 14:] = False
    frac = 0.9 if name == "masked_16x16" else 0.6   # (a padded pair keeps an 8 x 6 interior: plant more to keep 16 matches)
    if name != "unrelated":
        for b in range(n):   # planted among the valid cells
            v0, v1 = m0[b].flatten().nonzero().flatten(), m1[b].flatten().nonzero().flatten()
            k = int(frac * min(len(v0), len(v1)))
            src = v0[torch.randperm(len(v0), generator=g)[:k]]
            dst = v1[torch.randperm(len(v1), generator=g)[:k]]
            f1[b, dst] = f0[b, src] + 0.3 * torch.randn(k, c, generator=g)
    out = {"feat0": (f0 * math.sqrt(12.0)).contiguous(), "feat1": (f1 * math.sqrt(12.0)).contiguous(), "hw0": hw0, "hw1": hw1,
           "hw0_i": (8 * hw0[0], 8 * hw0[1])}
    if name == "masked_16x16":
        out.update(mask0=m0, mask1=m1, scale0=torch.tensor([[1.5, 0.75], [0.3, 2.5]]), scale1=torch.tensor([[0.6, 1.7], [2.0, 0.5]]))
    return out


# ---- LoFTR layers with full (softmax) attention ---------------------------------------------------------------------
# name: (stage, layer_names (None: ONE layer call, layers.0), n, L, S, seed, taps of the two outputs as (dim, step))
LOFTR_FULL_CASES = {
    "layer_self": ("coarse", None, 2, 200, 200, 41, ((1, 4), None)),
    "layer_cross": ("coarse", None, 2, 80, 200, 42, ((1, 1), None)),
    "coarse_xfmr": ("coarse", ["self", "cross"] * 2, 2, 80, 200, 43, ((1, 1), (1, 4))),
    "fine_xfmr": ("fine", ["self", "cross"], 37, 25, 25, 44, ((0, 4), (0, 4))),
}


def loftr_full_case(name):
    """Inputs of tests/golden/loftr_full.npz (scripts/gen_golden_loftr_full.py): dict(stage 'coarse' | 'fine', layer_names —
    None for one call of layers.0 —, feat0 [n, L, C], feat1 [n, S, C] or None (the layer updates feat0 against itself), taps:
    the (dim, step) stride with which each stored output is sampled).  Inputs are 3 * randn: under
    `synthetic_matcher_state_dict(0)` the softmax scores then have a standard deviation of ~9 and the median largest
    probability of a row is 0.84, so an online softmax really moves its running maximum."""
    stage, names, n, L, S, seed, taps = LOFTR_FULL_CASES[name]
    C = 256 if stage == "coarse" else 128
    g = torch.Generator().manual_seed(seed)
    f0 = 3.0 * torch.randn(n, L, C, generator=g)
    f1 = None if names is None and name.endswith("self") else 3.0 * torch.randn(n, S, C, generator=g)
    return {"stage": stage, "layer_names": names, "feat0": f0, "feat1": f1, "taps": taps}


def loftr_full_tap(t, tap):
    """The stored sample of an output of `loftr_full_case`: every step-th index along dim."""
    dim, step = tap
    return t[:, ::step] if dim == 1 else t[::step]


def loftr_full_matcher_case(name):
    """Image pairs of tests/golden/loftr_full_128.npz (Matcher with both transformers on full attention, thr 1e-3):
    'pairs128' = synthetic_gray_pairs(2, 128, 128, seed=21); '96x128_vs_128x96' = one pair of different shapes, image1 a fresh
    texture with a 96 x 96 region of image0 pasted 16 rows lower."""
    if name == "pairs128":
        return synthetic_gray_pairs(2, 128, 128, seed=21)
    if name == "96x128_vs_128x96":
        i0 = synthetic_gray_pairs(1, 96, 128, seed=21)[0]
        i1 = synthetic_gray_pairs(1, 128, 96, seed=22)[0]
        i1[:, :, 16:112, :] = i0[:, :, :, 16:112]
        return i0, i1.contiguous()
    raise KeyError(name)


# ---- SAM prompt encoder + mask decoder ---------------------------------------------------------------------------------
def synthetic_sam_decoder_state_dict(seed=0):
    """Seeded synthetic weights in the layout of a `Sam` checkpoint's `prompt_encoder.*` and `mask_decoder.*` keys
    (segment_anything/modeling/{prompt_encoder,mask_decoder,transformer}.py as build_sam.py builds them).  Linear and
    (transposed) convolution weights have std 1 / sqrt(fan_in), so every branch and the mask logits stay O(1)."""
    from .sam_decoder import MaskDecoder, PromptEncoder, TwoWayTransformer
    g = torch.Generator().manual_seed(seed)
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16)
    md = MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(depth=2, embedding_dim=256, num_heads=8, mlp_dim=2048),
                     num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256)
    sd = {}
    for prefix, model in (("prompt_encoder.", pe), ("mask_decoder.", md)):
        for mname, m in model.named_modules():
            for pname, t in list(m.named_parameters(recurse=False)) + list(m.named_buffers(recurse=False)):
                key = prefix + (mname + "." if mname else "") + pname
                shape = tuple(t.shape)
                if isinstance(m, (torch.nn.LayerNorm,)) or type(m).__name__ == "LayerNorm2d":
                    v = (1.0 + 0.1 * torch.randn(shape, generator=g)) if pname == "weight" else 0.05 * torch.randn(shape, generator=g)
                elif pname == "bias":
                    v = 0.1 * torch.randn(shape, generator=g)
                elif isinstance(m, torch.nn.Linear):
                    v = torch.randn(shape, generator=g) / math.sqrt(shape[1])
                elif isinstance(m, torch.nn.ConvTranspose2d):
                    v = torch.randn(shape, generator=g) / math.sqrt(shape[0])
                elif isinstance(m, torch.nn.Conv2d):
                    v = torch.randn(shape, generator=g) / math.sqrt(shape[1] * shape[2] * shape[3])
                else:   # embeddings, the Gaussian frequency matrix
                    v = torch.randn(shape, generator=g)
                sd[key] = v.float().contiguous()
    return sd


def synthetic_sam_image_embedding(seed=0):
    """A seeded unit-scale image embedding [1, 256, 64, 64] (what the SAM image encoder hands the decoder)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 256, 64, 64, generator=g, dtype=torch.float32)


SAM_DECODER_CASES = ("grid", "box")


def sam_decoder_case(name):
    """Prompts of the decoder fixtures: (points (coords, labels) or None, boxes or None, multimask_output).
    "grid": SamAutomaticMaskGenerator's 16 x 16 point grid of a 480 x 640 frame, mapped into the 1024 frame as
    ResizeLongestSide.apply_coords maps it (float64, as the generator hands them to predict_torch), label 1, one point per
    prompt (the prompt encoder adds the padding point).  "box": 6 prompts of two points (labels 1 / 0) and a box."""
    import numpy as np
    if name == "grid":
        n, h, w = 16, 480, 640
        off = 1 / (2 * n)
        side = np.linspace(off, 1 - off, n)
        xs, ys = np.tile(side[None, :], (n, 1)), np.tile(side[:, None], (1, n))
        pts = np.stack([xs, ys], axis=-1).reshape(-1, 2) * np.array([w, h])[None, :]
        scale = 1024 * 1.0 / max(h, w)
        nh, nw = int(h * scale + 0.5), int(w * scale + 0.5)
        pts = pts.astype(float)
        pts[..., 0] = pts[..., 0] * (nw / w)
        pts[..., 1] = pts[..., 1] * (nh / h)
        coords = torch.as_tensor(pts)[:, None, :]
        labels = torch.ones(coords.shape[0], dtype=torch.int)[:, None]
        return (coords, labels), None, True
    if name == "box":
        g = torch.Generator().manual_seed(17)
        coords = torch.rand(6, 2, 2, generator=g) * torch.tensor([1024.0, 768.0])
        labels = torch.tensor([[1, 0]] * 6, dtype=torch.int)
        lo = torch.rand(6, 2, generator=g) * torch.tensor([600.0, 400.0])
        boxes = torch.cat([lo, lo + 100 + torch.rand(6, 2, generator=g) * 300], dim=1)
        return (coords, labels), boxes, False
    raise KeyError(name)


def sam_forward_case(device="cpu"):
    """A seeded `batched_input` of `Sam.forward` (modeling/sam.py:53-131): two records whose images differ in shape and whose
    prompts differ in kind.  Record 0: a 3 x 768 x 1024 image (original 480 x 640) with 2 boxes; record 1: a 3 x 1024 x 683
    image (original 600 x 400) with `point_coords` [3, 2, 2] and labels 1 / 0.  Pixel values are floats in 0 .. 255 (smooth
    gradients plus noise); prompts are in the input frame."""
    g = torch.Generator().manual_seed(23)

    def image(h, w):
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) / h, torch.arange(w, dtype=torch.float32) / w, indexing="ij")
        base = torch.stack([yy, xx, 0.5 * (yy + xx)]) * 160.0 + 40.0
        return (base + 25.0 * torch.randn(3, h, w, generator=g)).clamp_(0.0, 255.0).contiguous()

    img0, img1 = image(768, 1024), image(1024, 683)
    lo = torch.rand(2, 2, generator=g) * torch.tensor([600.0, 400.0])
    boxes = torch.cat([lo, lo + 100 + torch.rand(2, 2, generator=g) * 250], dim=1)
    coords = torch.rand(3, 2, 2, generator=g) * torch.tensor([683.0, 1024.0])
    labels = torch.tensor([[1, 0]] * 3, dtype=torch.int)
    return [{"image": img0.to(device), "original_size": (480, 640), "boxes": boxes.to(device)},
            {"image": img1.to(device), "original_size": (600, 400), "point_coords": coords.to(device),
             "point_labels": labels.to(device)}]


SAM_MASK_PROMPT_CASES = {"box": (6, 0), "points": (17, 1)}   # name -> (P, seed of the masks): tests/golden/sam_mask_prompt.npz


def sam_mask_prompt_case(P, seed=0):
    """Seeded mask prompts [P, 1, 256, 256] fp32 that look like the decoder's low-res logits (what `predict(mask_input=)` is fed):
    a floor of -8, three Gaussian blobs of amplitude 16 with sigma uniform in 10 .. 60 px at uniform centres, and noise of
    std 0.5; all from one CPU generator (per prompt: the centres, the sigmas, then the noise)."""
    g = torch.Generator().manual_seed(seed)
    n = 256
    yy, xx = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    out = torch.empty(P, 1, n, n)
    for p in range(P):
        centre = torch.rand(3, 2, generator=g) * n
        sigma = 10.0 + 50.0 * torch.rand(3, generator=g)
        m = torch.full((n, n), -8.0)
        for (cy, cx), s in zip(centre.tolist(), sigma.tolist()):
            m += 16.0 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
        out[p, 0] = m + 0.5 * torch.randn(n, n, generator=g)
    return out.contiguous()


def sam_mask_prompt_inputs(name):
    """The prompts of fixture case `name`: (points or None, boxes or None, masks, multimask_output).  "box": the 6 prompts of
    `sam_decoder_case("box")` (two points and a box each) plus 6 masks, single-mask output; "points": 17 prompts of one
    positive point each (every 15th of the "grid" case) plus 17 masks, multimask output."""
    P, seed = SAM_MASK_PROMPT_CASES[name]
    masks = sam_mask_prompt_case(P, seed)
    if name == "box":
        points, boxes, _ = sam_decoder_case("box")
        return points, boxes, masks, False
    (coords, labels), _, _ = sam_decoder_case("grid")
    return (coords[::15][:P].contiguous(), labels[::15][:P].contiguous()), None, masks, True


# ---- SAM automatic mask generator: post-processing ---------------------------------------------------------------------
# name -> (M masks, frame (H, W)); the resized frame inside the 1024 square follows from ResizeLongestSide
SAM_GENERATOR_CASES = {"frame": (128, (480, 640)), "portrait": (48, (333, 332))}


def sam_generator_case(name, M=None):
    """Seeded inputs of the generator's post-processing fixtures: (low_res [M, 256, 256] fp32, iou_preds [M] fp32,
    input_size (ih, iw), original_size (H, W)).  A mask's logits are a negative floor with one to three flat-topped blobs of
    +-12 (the steepness of their rims varies, so stability scores spread around 0.95), small satellite blobs and pin holes
    (islands and holes on either side of 250 pixels) and low-amplitude noise.  Blob centres come from a small pool so
    that near-duplicate masks exist for NMS; some masks have no blob (empty after thresholding) and some sit on the frame
    border.  `iou_preds` are drawn around 0.9, all distinct."""
    M0, (H, W) = SAM_GENERATOR_CASES[name]
    M = M or M0          # a larger M (timing runs) extends the same seeded sequence
    g = torch.Generator().manual_seed({"frame": 101, "portrait": 202}[name])
    scale = 1024.0 / max(H, W)
    ih, iw = int(H * scale + 0.5), int(W * scale + 0.5)
    n = 256
    fy, fx = ih / 1024.0, iw / 1024.0          # the part of the low-res square the frame covers
    yy, xx = torch.meshgrid(torch.arange(n, dtype=torch.float32) / n, torch.arange(n, dtype=torch.float32) / n, indexing="ij")
    u = lambda *s: torch.rand(*s, generator=g)
    pool = torch.stack([u(24) * fy, u(24) * fx], 1)
    pool[:4, 0] = torch.tensor([0.0, fy, 0.5 * fy, fy])     # four centres on the frame border (fy / fx: its far edges)
    pool[:4, 1] = torch.tensor([0.5 * fx, 0.4 * fx, fx, fx])
    low = torch.empty(M, n, n)

    def disc(cy, cx, ry, rx, gain):
        """A flat-topped blob: `gain` logits per radius across its rim, clamped to +-12."""
        d = torch.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        return (gain * (1.0 - d)).clamp_(-12.0, 12.0)

    for i in range(M):
        z = torch.full((n, n), -12.0)
        if i % 16 != 7:                          # every sixteenth mask stays empty
            c = pool[int(torch.randint(0, 24, (1,), generator=g))]
            k = 1 + int(torch.randint(0, 3, (1,), generator=g))
            gain = 30.0 * 8.0 ** u(1).item()     # 30 .. 240: stability roughly 1 - 4 / gain
            for b in range(k):
                cy = c[0] + (0.0 if b == 0 else (u(1).item() - 0.5) * 0.2)
                cx = c[1] + (0.0 if b == 0 else (u(1).item() - 0.5) * 0.2)
                z = torch.maximum(z, disc(cy, cx, 0.05 + 0.15 * u(1).item(), 0.05 + 0.15 * u(1).item(), gain))
            for _ in range(int(torch.randint(0, 4, (1,), generator=g))):   # satellites: islands, or holes in the blobs
                r = (2.0 + 4.0 * u(1).item()) / n
                if u(1).item() < 0.5:
                    z = torch.maximum(z, disc(u(1).item() * fy, u(1).item() * fx, r, r, 24.0))
                else:
                    z = torch.minimum(z, -disc(c[0] + (u(1).item() - 0.5) * 0.08, c[1] + (u(1).item() - 0.5) * 0.08, r, r, 24.0))
        low[i] = z + 0.25 * torch.randn(n, n, generator=g)
    iou = (0.9 + 0.05 * torch.randn(M, generator=g)).float()
    assert iou.unique().numel() == M
    return low.contiguous(), iou.contiguous(), (ih, iw), (H, W)


# ---- learned pose regressor (pose/model.py:Mkpts_Reg_Model) -------------------------------------------------------------------

POSE_REGRESSOR_MODES = {"matrix": 9, "quat": 4, "6d": 6}
# (num_sample, pairs per call) of tests/golden/pose_regressor.npz; every mode at each; the last pair of a call with more than
# one pair has zero-padded rows.  The (300, 2) case is there for the real mlp.0 width and its 64-bit indexing (mode 'matrix' only)
POSE_REGRESSOR_CASES = [(S, B) for S in (5, 37, 70) for B in (1, 3, 5)]
POSE_REGRESSOR_LARGE = (300, 2)


def pose_regressor_keys(num_sample, mode="matrix"):
    """The 78 state-dict keys of `Mkpts_Reg_Model(num_sample, mode)` with their shapes, in the reference's order."""
    S, d, hid = int(num_sample), 76, 2048
    layer = [("self_attn.in_proj_weight", (3 * d, d)), ("self_attn.in_proj_bias", (3 * d,)), ("self_attn.out_proj.weight", (d, d)),
             ("self_attn.out_proj.bias", (d,)), ("linear1.weight", (hid, d)), ("linear1.bias", (hid,)), ("linear2.weight", (d, hid)),
             ("linear2.bias", (d,)), ("norm1.weight", (d,)), ("norm1.bias", (d,)), ("norm2.weight", (d,)), ("norm2.bias", (d,))]
    keys = [("transformerlayer." + k, s) for k, s in layer]
    for i in range(4):
        keys += [(f"transformer.layers.{i}.{k}", s) for k, s in layer]
    keys += [("translation_head.weight", (3, 32)), ("translation_head.bias", (3,))]
    r = POSE_REGRESSOR_MODES[mode]
    keys += [("rotation_head.weight", (r, 32)), ("rotation_head.bias", (r,))]
    widths = [76 * S, 19 * S, S, 256, 128, 64, 32, 32]
    for i in range(7):
        keys += [(f"mlp.{3 * i}.weight", (widths[i + 1], widths[i])), (f"mlp.{3 * i}.bias", (widths[i + 1],))]
    return keys


def pose_regressor_state_dict(num_sample, mode="matrix", seed=0):
    """Seeded weights that keep every branch O(1): matrices N(0, 2 / fan_in), biases and LayerNorm offsets N(0, 0.3^2), LayerNorm
    gains 1 + N(0, 0.3^2).  (With torch's default init the outputs barely react to the inputs.)  The rotation head is drawn from
    a generator of its own, so the three modes share every other tensor."""
    g = torch.Generator().manual_seed(1000 + seed)
    gr = torch.Generator().manual_seed(2000 + seed)
    sd = {}
    for k, shape in pose_regressor_keys(num_sample, mode):
        gen = gr if k.startswith("rotation_head") else g
        if len(shape) == 2:
            sd[k] = torch.randn(shape, generator=gen) * (2.0 / shape[1]) ** 0.5
        elif "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.3 * torch.randn(shape, generator=gen)
        else:
            sd[k] = 0.3 * torch.randn(shape, generator=gen)
    return sd


def pose_regressor_matches(counts, seed=0, hw=(480, 640)):
    """Seeded matches of len(counts) pairs in the matcher's compacted layout: (kpts0, kpts1) [sum(counts), 2] fp32 pixel
    coordinates on a quarter-pixel grid (x < hw[1], y < hw[0]), kpts1 = kpts0 moved by a per-pair shift plus jitter."""
    g = torch.Generator().manual_seed(3000 + seed)
    k0, k1 = [], []
    for c in counts:
        c = max(int(c), 0)
        p = torch.rand(c, 2, generator=g) * torch.tensor([hw[1] - 1.0, hw[0] - 1.0])
        shift = (torch.rand(1, 2, generator=g) - 0.5) * 80.0
        q = (p + shift + torch.randn(c, 2, generator=g)).clamp_(min=0.0)
        q = torch.minimum(q, torch.tensor([hw[1] - 1.0, hw[0] - 1.0]))
        k0.append(torch.round(p * 4) / 4)
        k1.append(torch.round(q * 4) / 4)
    return torch.cat(k0).float(), torch.cat(k1).float()


def pose_regressor_case(num_sample, n_pairs, seed=None):
    """Dense inputs of one fixture case: (mkpts0, mkpts1) [B, S, 2]; the last pair of a call of several keeps 2 S / 3 rows, the rest
    of its rows are zero padding."""
    S, B = int(num_sample), int(n_pairs)
    counts = [S] * B
    if B > 1:
        counts[-1] = max(1, 2 * S // 3)
    k0, k1 = pose_regressor_matches(counts, seed=100 * S + B if seed is None else seed)
    d0, d1 = torch.zeros(B, S, 2), torch.zeros(B, S, 2)
    off = 0
    for b, c in enumerate(counts):
        d0[b, :c], d1[b, :c] = k0[off:off + c], k1[off:off + c]
        off += c
    return d0, d1


def pose_regressor_tap_slots(num_sample):
    """Sample slots of the embedding / encoder taps the fixture keeps (all pairs of the call at each)."""
    S = int(num_sample)
    return sorted({s for s in (0, 1, S // 2, 31, 32, 33, 63, 64, 65, 2 * S // 3 - 1, 2 * S // 3, S - 1) if 0 <= s < S})


# ---- ConvNeXtV2 backbone and the image pose head (pose/convnextv2/convnextv2.py, pose/model_cnn.py) ---------------------------

CONVNEXT_SMALL = dict(depths=[1, 1, 2, 1], dims=[64, 80, 160, 320], num_classes=32)
CONVNEXT_TINY = dict(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], num_classes=1000)
# tests/golden/convnext.npz.  small: a non-square last map of 3 x 5, smaller than the 7 x 7 kernel, and the K % 32 != 0 route (80);
# tiny_full: convnextv2_tiny at full depth on two 64 x 64 images side by side; pose_*: the small trunk under the two pose heads
CONVNEXT_CASES = {"small": (CONVNEXT_SMALL, 3, (96, 160), 0), "tiny_full": (CONVNEXT_TINY, 2, (64, 128), 1)}
CONVNEXT_POSE_CASES = {f"pose_{m}": (m, 2, (96, 80), 2) for m in POSE_REGRESSOR_MODES}
CONVNEXT_TAP_SAMPLES = 4096     # entries kept of a tap wider than that, at seeded flat positions


def convnext_keys(depths, dims, num_classes):
    """State-dict keys of `ConvNeXtV2(depths=, dims=, num_classes=)` with their shapes, in the reference's order."""
    keys = [("downsample_layers.0.0.weight", (dims[0], 3, 4, 4)), ("downsample_layers.0.0.bias", (dims[0],)),
            ("downsample_layers.0.1.weight", (dims[0],)), ("downsample_layers.0.1.bias", (dims[0],))]
    for i in range(3):
        keys += [(f"downsample_layers.{i + 1}.0.weight", (dims[i],)), (f"downsample_layers.{i + 1}.0.bias", (dims[i],)),
                 (f"downsample_layers.{i + 1}.1.weight", (dims[i + 1], dims[i], 2, 2)), (f"downsample_layers.{i + 1}.1.bias", (dims[i + 1],))]
    for i in range(4):
        c = dims[i]
        for j in range(depths[i]):
            p = f"stages.{i}.{j}."
            keys += [(p + "dwconv.weight", (c, 1, 7, 7)), (p + "dwconv.bias", (c,)), (p + "norm.weight", (c,)), (p + "norm.bias", (c,)),
                     (p + "pwconv1.weight", (4 * c, c)), (p + "pwconv1.bias", (4 * c,)), (p + "grn.gamma", (1, 1, 1, 4 * c)),
                     (p + "grn.beta", (1, 1, 1, 4 * c)), (p + "pwconv2.weight", (c, 4 * c)), (p + "pwconv2.bias", (c,))]
    keys += [("norm.weight", (dims[3],)), ("norm.bias", (dims[3],)), ("head.weight", (num_classes, dims[3])), ("head.bias", (num_classes,))]
    return keys


def _convnext_tensor(k, shape, gen):
    if k.endswith("grn.gamma"):
        return 0.5 + torch.rand(shape, generator=gen)
    if k.endswith("grn.beta"):
        return 0.3 * torch.randn(shape, generator=gen)
    if len(shape) >= 2:                                   # matrices and convolution kernels: 1.5 / sqrt(fan_in)
        return torch.randn(shape, generator=gen) * (1.5 / math.prod(shape[1:]) ** 0.5)
    if k.endswith("bias"):
        return 0.2 * torch.randn(shape, generator=gen)
    return 1.0 + 0.3 * torch.randn(shape, generator=gen)  # LayerNorm gains


def convnext_state_dict(depths, dims, num_classes, seed=0):
    """Seeded weights with every term alive (torch's default init leaves GRN at zero and the branches at 0.02): GRN gamma in
    [0.5, 1.5], beta 0.3 N; biases 0.2 N; LayerNorm gains 1 + 0.3 N; matrices and kernels 1.5 / sqrt(fan_in) N."""
    g = torch.Generator().manual_seed(4000 + seed)
    return {k: _convnext_tensor(k, s, g) for k, s in convnext_keys(depths, dims, num_classes)}


def convnext_pose_state_dict(mode, seed=0):
    """`pose/model_cnn.py:Mkpts_Reg_Model` over the small trunk: `convnextv2.model.*` and the two heads; the rotation head from a
    generator of its own, so the modes share every other tensor."""
    sd = {"convnextv2.model." + k: v for k, v in convnext_state_dict(seed=seed, **CONVNEXT_SMALL).items()}
    g, gr = torch.Generator().manual_seed(5000 + seed), torch.Generator().manual_seed(6000 + seed)
    r = POSE_REGRESSOR_MODES[mode]
    for k, shape, gen in (("translation_head_rot.weight", (3, 32), g), ("translation_head_rot.bias", (3,), g),
                          ("rotation_head_rot.weight", (r, 32), gr), ("rotation_head_rot.bias", (r,), gr)):
        sd[k] = _convnext_tensor(k, shape, gen)
    return sd


def convnext_case(name):
    """One case of tests/golden/convnext.npz: dict(cfg, state_dict, x [B, 3, H, W]) for the backbone cases, dict(mode, state_dict,
    img0, img1 [B, 3, H, W / 2 each], cfg) for the pose cases."""
    if name in CONVNEXT_CASES:
        cfg, B, (H, W), seed = CONVNEXT_CASES[name]
        g = torch.Generator().manual_seed(7000 + seed)
        return {"cfg": cfg, "state_dict": convnext_state_dict(seed=seed, **cfg), "x": torch.randn(B, 3, H, W, generator=g)}
    mode, B, (H, W), seed = CONVNEXT_POSE_CASES[name]
    g = torch.Generator().manual_seed(7000 + seed)
    return {"cfg": CONVNEXT_SMALL, "mode": mode, "state_dict": convnext_pose_state_dict(mode, seed=seed),
            "img0": torch.randn(B, 3, H, W, generator=g), "img1": torch.randn(B, 3, H, W, generator=g)}


def convnext_tap_index(name, tap, numel):
    """Flat positions of a tap the fixture keeps: all of it up to CONVNEXT_TAP_SAMPLES entries, else that many seeded positions."""
    if numel <= CONVNEXT_TAP_SAMPLES:
        return torch.arange(numel)
    g = torch.Generator().manual_seed(8000 + sum(map(ord, name + tap)))
    return torch.randperm(numel, generator=g)[:CONVNEXT_TAP_SAMPLES].sort().values


CONVNEXT_TAPS = ("stem", "stage0", "stage1", "stage2", "stage3", "features", "logits")


def fcmae_checkpoint(seed=0):
    """A seeded FCMAE-style (sparse pre-training) checkpoint dict of a two-block toy encoder, for `remap_checkpoint_keys`."""
    g = torch.Generator().manual_seed(9000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ck = {"encoder.downsample_layers.0.0.weight": r(8, 3, 4, 4), "encoder.downsample_layers.0.0.bias": r(8),
          "encoder.downsample_layers.0.1.weight": r(8), "encoder.downsample_layers.0.1.bias": r(8),
          "encoder.downsample_layers.1.0.ln.weight": r(8), "encoder.downsample_layers.1.0.ln.bias": r(8),
          "encoder.downsample_layers.1.1.kernel": r(4, 8, 16), "encoder.downsample_layers.1.1.bias": r(1, 16)}
    for i, c in ((0, 8), (1, 16)):
        p = f"encoder.stages.{i}.0."
        ck.update({p + "dwconv.kernel": r(49, c), p + "dwconv.bias": r(1, c), p + "norm.ln.weight": r(c), p + "norm.ln.bias": r(c),
                   p + "pwconv1.linear.weight": r(4 * c, c), p + "pwconv1.linear.bias": r(4 * c), p + "grn.gamma": r(1, 4 * c),
                   p + "grn.beta": r(1, 4 * c), p + "pwconv2.linear.weight": r(c, 4 * c), p + "pwconv2.linear.bias": r(c)})
    ck["norm.weight"], ck["norm.bias"] = r(16), r(16)
    return ck


# ---- MoCoPE fusion pose model (pose/model0604.py:MoCoPE) ----------------------------------------------------------------------

MOCOPE_TRAIN_TYPES = ("mkpts+cnn", "mkpts", "cnn")
# tests/golden/mocope.npz: (num_sample, pairs per call); every mode at MOCOPE_MODES_AT, '6d' elsewhere; the reduced train types at
# MOCOPE_REDUCED; MOCOPE_WIDE for mlp1.0 = [8360, 16720] (flat index past 2^27).  Images are MOCOPE_IMAGE x MOCOPE_IMAGE, the trunk
# is CONVNEXT_SMALL with the 1000-class head MoCoPE reads.
MOCOPE_CASES = [(S, B) for S in (5, 37, 70) for B in (1, 2, 3, 5)]
MOCOPE_MODES_AT = 37
MOCOPE_REDUCED = (37, 3)
MOCOPE_WIDE = (220, 2)
MOCOPE_IMAGE = 64
MOCOPE_TRUNK = dict(CONVNEXT_SMALL, num_classes=1000)
MOCOPE_TAPS = ("embedding", "memory", "transformer_mkpts", "x_mkpts", "x_img", "qmkpts", "qimg")
MOCOPE_TAP_COLUMNS = list(range(0, 512, 9))       # columns the fixture keeps of the [B, 2, 512] taps (all rows)
MOCOPE_TAPS_OF = {"mkpts+cnn": MOCOPE_TAPS, "mkpts": ("embedding", "memory", "transformer_mkpts", "x_mkpts", "qmkpts"),
                  "cnn": ("x_img", "qimg")}


def _transformer_keys(prefix, d, hid=2048):
    attn = lambda a: [(f"{a}.in_proj_weight", (3 * d, d)), (f"{a}.in_proj_bias", (3 * d,)), (f"{a}.out_proj.weight", (d, d)),  # noqa: E731
                      (f"{a}.out_proj.bias", (d,))]
    ffn = [("linear1.weight", (hid, d)), ("linear1.bias", (hid,)), ("linear2.weight", (d, hid)), ("linear2.bias", (d,))]
    norms = lambda n: [(f"norm{i + 1}.{k}", (d,)) for i in range(n) for k in ("weight", "bias")]  # noqa: E731
    keys = []
    for i in range(6):
        keys += [(f"{prefix}.encoder.layers.{i}.{k}", s) for k, s in attn("self_attn") + ffn + norms(2)]
    keys += [(f"{prefix}.encoder.norm.weight", (d,)), (f"{prefix}.encoder.norm.bias", (d,))]
    for i in range(6):
        keys += [(f"{prefix}.decoder.layers.{i}.{k}", s) for k, s in attn("self_attn") + attn("multihead_attn") + ffn + norms(3)]
    keys += [(f"{prefix}.decoder.norm.weight", (d,)), (f"{prefix}.decoder.norm.bias", (d,))]
    return keys


def mocope_keys(num_sample, mode="6d"):
    """The state-dict keys of `MoCoPE(num_sample, mode)` outside `convnextv2.model.*`, with their shapes, in the reference's order."""
    S = int(num_sample)
    keys = _transformer_keys("transformer_mkpts", 76)
    keys += [("mlp1.0.weight", (38 * S, 76 * S)), ("mlp1.0.bias", (38 * S,)), ("mlp1.3.weight", (1024, 38 * S)), ("mlp1.3.bias", (1024,))]
    keys += [("mlp_img.0.weight", (512, 1000)), ("mlp_img.0.bias", (512,))]
    keys += _transformer_keys("mkpts_as_q", 512) + _transformer_keys("cnn_as_q", 512)
    widths = [2048, 1024, 512, 256, 128, 64, 32, 32]
    for i in range(7):
        keys += [(f"mlp2.{3 * i}.weight", (widths[i + 1], widths[i])), (f"mlp2.{3 * i}.bias", (widths[i + 1],))]
    r = POSE_REGRESSOR_MODES[mode]
    keys += [("translation_head.weight", (3, 32)), ("translation_head.bias", (3,)), ("rotation_head.weight", (r, 32)),
             ("rotation_head.bias", (r,))]
    return keys


def mocope_state_dict(num_sample, mode="6d", seed=0):
    """Seeded weights of the whole model, `convnextv2.model.*` (the MOCOPE_TRUNK) included, that keep every branch O(1): the rule of
    `pose_regressor_state_dict`.  Every tensor outside the rotation head and mlp1 has a generator of its own group, so neither the
    mode nor num_sample changes the others."""
    gens = {}

    def gen(k):
        group = "rotation_head" if k.startswith("rotation_head") else "mlp1" if k.startswith("mlp1") else "rest"
        if group not in gens:
            gens[group] = torch.Generator().manual_seed(10000 + 1000 * ("rotation_head", "mlp1", "rest").index(group) + seed)
        return gens[group]

    sd = {}
    for k, shape in mocope_keys(num_sample, mode):
        if len(shape) == 2:
            sd[k] = torch.randn(shape, generator=gen(k)) * (2.0 / shape[1]) ** 0.5
        elif "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.3 * torch.randn(shape, generator=gen(k))
        else:
            sd[k] = 0.3 * torch.randn(shape, generator=gen(k))
    sd.update({"convnextv2.model." + k: v for k, v in convnext_state_dict(seed=seed, **MOCOPE_TRUNK).items()})
    return sd


def mocope_case(num_sample, n_pairs):
    """Inputs of one fixture case: (mkpts0, mkpts1 [B, S, 2] as `pose_regressor_case`, img0, img1 [B, 3, 64, 64])."""
    d0, d1 = pose_regressor_case(num_sample, n_pairs)
    g = torch.Generator().manual_seed(11000 + 100 * int(num_sample) + int(n_pairs))
    shape = (int(n_pairs), 3, MOCOPE_IMAGE, MOCOPE_IMAGE)
    return d0, d1, torch.randn(shape, generator=g), torch.randn(shape, generator=g)


# ---- Vision Mamba (pope_amd/vim.py; tests/golden/vim.npz) ------------------------------------------------------------------------
VIM_TINY = dict(embed_dim=192, depth=24)
VIM_SMALL = dict(embed_dim=384, depth=24)
# name -> (width settings, stride, img_size, num_classes, B, seed).  small_s8 is the fork's default
# (vim_small_patch16_stride8_224_..., L = 730); small_s8_64: 7 x 7 patches, L = 50, shorter than one scan chunk
VIM_CASES = {"tiny_s16": (VIM_TINY, 16, 224, 100, 2, 0), "small_s8": (VIM_SMALL, 8, 224, 1000, 2, 1),
             "small_s16": (VIM_SMALL, 16, 224, 100, 1, 2), "small_s8_64": (VIM_SMALL, 8, 64, 100, 3, 3)}
VIM_TAPS = ("tokens", "layer0", "layer11", "layer23", "features", "logits")
VIM_TAP_SAMPLES = 1024          # entries kept of a tap wider than that, at seeded flat positions
VIM_D_STATE, VIM_D_CONV = 16, 4


def vim_geometry(img_size, stride):
    """(g, L, class-token row) of a square image: g = (img - 16) // stride + 1 patches per side, L = g g + 1 tokens."""
    g = (img_size - 16) // stride + 1
    return g, g * g + 1, (g * g) // 2


def vim_keys(embed_dim, depth, num_classes, img_size=224, stride=16):
    """State-dict keys of the four registered `VisionMamba` factories' configuration with their shapes, in the reference's order:
    a module's own parameters come before its children's, so a mixer lists A_log, D, A_b_log, D_b first."""
    d, e, n = embed_dim, 2 * embed_dim, VIM_D_STATE
    r = -(-d // 16)
    _, L, _ = vim_geometry(img_size, stride)
    keys = [("cls_token", (1, 1, d)), ("pos_embed", (1, L, d)), ("patch_embed.proj.weight", (d, 3, 16, 16)), ("patch_embed.proj.bias", (d,)),
            ("head.weight", (num_classes, d)), ("head.bias", (num_classes,))]
    for i in range(depth):
        p = f"layers.{i}.mixer."
        keys += [(p + "A_log", (e, n)), (p + "D", (e,)), (p + "A_b_log", (e, n)), (p + "D_b", (e,)), (p + "in_proj.weight", (2 * e, d)),
                 (p + "conv1d.weight", (e, 1, VIM_D_CONV)), (p + "conv1d.bias", (e,)), (p + "x_proj.weight", (r + 2 * n, e)),
                 (p + "dt_proj.weight", (e, r)), (p + "dt_proj.bias", (e,)), (p + "conv1d_b.weight", (e, 1, VIM_D_CONV)),
                 (p + "conv1d_b.bias", (e,)), (p + "x_proj_b.weight", (r + 2 * n, e)), (p + "dt_proj_b.weight", (e, r)),
                 (p + "dt_proj_b.bias", (e,)), (p + "out_proj.weight", (d, e)), (f"layers.{i}.norm.weight", (d,))]
    keys += [("norm_f.weight", (d,))]
    return keys


def _vim_tensor(k, shape, gen):
    leaf = k.split(".")[-1] if k.split(".")[-1] not in ("weight", "bias") else ".".join(k.split(".")[-2:])
    if leaf in ("A_log", "A_b_log"):        # A = -(1 .. 16) f, f per channel in [0.5, 2] (log-uniform)
        f = torch.exp(torch.rand(shape[0], 1, generator=gen) * math.log(4.0) + math.log(0.5))
        return torch.log(torch.arange(1, shape[1] + 1, dtype=torch.float32)[None, :] * f)
    if leaf in ("D", "D_b"):
        return 1.0 + 0.3 * torch.randn(shape, generator=gen)
    if leaf in ("dt_proj.bias", "dt_proj_b.bias"):   # softplus^-1 of log-uniform [1e-3, 1e-1]
        dt = torch.exp(torch.rand(shape, generator=gen) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
        return dt + torch.log(-torch.expm1(-dt))
    if leaf in ("conv1d.weight", "conv1d_b.weight"):
        return 0.5 * torch.randn(shape, generator=gen)
    if leaf in ("cls_token", "pos_embed"):
        return torch.randn(shape, generator=gen)
    if leaf in ("dt_proj.weight", "dt_proj_b.weight"):
        return torch.randn(shape, generator=gen) * (2.0 / shape[1] ** 0.5)
    if leaf == "out_proj.weight":           # the gated scan output has an rms of about 8 (long memories: delta |A| is small)
        return torch.randn(shape, generator=gen) * (0.12 / shape[1] ** 0.5)
    if len(shape) >= 2:                     # in_proj, x_proj, patch kernel, head: 1.5 / sqrt(fan_in)
        return torch.randn(shape, generator=gen) * (1.5 / math.prod(shape[1:]) ** 0.5)
    if leaf.endswith("bias"):
        return 0.2 * torch.randn(shape, generator=gen)
    return 1.0 + 0.3 * torch.randn(shape, generator=gen)    # RMSNorm gains


def vim_state_dict(embed_dim, depth, num_classes, img_size=224, stride=16, seed=0):
    """Seeded weights with every term of the mixer alive (the reference's init leaves out_proj at 1 / sqrt(depth) of a 0.02
    branch): A = -(1 .. 16) f with f in [0.5, 2] per channel, dt_proj.bias the inverse softplus of log-uniform [1e-3, 1e-1],
    D = 1 + 0.3 N, conv taps 0.5 N, pos_embed / cls_token N, the `_b` tensors drawn after and independently of the forward
    ones, matrices scaled so that a block's mixer output is of order 1 against an order-1 residual."""
    g = torch.Generator().manual_seed(9000 + seed)
    return {k: _vim_tensor(k, s, g) for k, s in vim_keys(embed_dim, depth, num_classes, img_size, stride)}


def vim_case(name):
    """One case of tests/golden/vim.npz: dict(cfg (VisionMamba keyword arguments), state_dict, x [B, 3, S, S])."""
    width, stride, img, ncls, B, seed = VIM_CASES[name]
    g = torch.Generator().manual_seed(9500 + seed)
    cfg = dict(width, stride=stride, img_size=img, num_classes=ncls)
    return {"cfg": cfg, "state_dict": vim_state_dict(width["embed_dim"], width["depth"], ncls, img, stride, seed=seed),
            "x": torch.randn(B, 3, img, img, generator=g)}


def vim_tap_index(name, tap, numel):
    """Flat positions of a tap the fixture keeps: all of it up to VIM_TAP_SAMPLES entries, else that many seeded positions."""
    if numel <= VIM_TAP_SAMPLES:
        return torch.arange(numel)
    g = torch.Generator().manual_seed(9800 + sum(map(ord, name + tap)))
    return torch.randperm(numel, generator=g)[:VIM_TAP_SAMPLES].sort().values


def vim_pos_embed_checkpoint(embed_dim=384, orig_size=14, num_classes=1000, seed=0):
    """A seeded stand-in for a released Vim checkpoint as the `Vim` loader sees it: {'model': {pos_embed of a 14 x 14 grid + class
    token, head.* of `num_classes`}}; the other keys are left to the model's own values (the loader is strict=False)."""
    g = torch.Generator().manual_seed(9900 + seed)
    return {"model": {"pos_embed": torch.randn(1, orig_size * orig_size + 1, embed_dim, generator=g),
                      "head.weight": torch.randn(num_classes, embed_dim, generator=g) * 0.05,
                      "head.bias": torch.randn(num_classes, generator=g) * 0.05}}
