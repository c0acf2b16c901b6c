"""Times of the Vision Mamba backbone (pope_amd/vim.py) on the GPU: the fork's default (small, stride 8, 224 x 224, L = 730) at
B = 2 and B = 48 (24 image pairs), per precision — the whole forward, one layer's launches one by one through the op-level
entries (add + RMSNorm, in_proj, conv1d + SiLU, the two x_proj, the scan, out_proj), the remainder (patch embedding, head, the
final norm), and an eager PyTorch restatement of the same model on the same card (a Python loop over the 730 time steps).

Every time is a device-event time over a window of repeated calls after a warm-up; the scan's memory floor is computed from
the shapes: 5 fp32 streams of B L E (the two conv outputs, z, the output, and one more for what a direction re-reads) plus the
x_proj rows B L (R + 32) of both directions, over the 8 TB/s HBM peak.

  python scripts/vim_time.py [--out profiles/vim_times.json] [--batches 2,48] [--no-eager]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import _lib, synth, vim  # noqa: E402

HBM_BYTES_PER_S = 8.0e12     # MI355X peak
N = 16


def event_ms(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def layer_ops(model, B, precision):
    """name -> closure of one launch of layer 0 at batch B, on buffers of the model's shapes."""
    lib = _lib.lib()
    w = model._weights(precision)
    k = w.layers_host[0]
    d, L = model.embed_dim, model.patch_embed.num_patches + 1
    e, r, M = 2 * d, -(-d // 16), B * L
    x3 = precision == "f16x3"
    prec = _lib.PRECISIONS[precision]
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    hid = torch.randn(M, d, generator=g).to(dev)
    res = torch.randn(M, d, generator=g).to(dev)
    op = torch.zeros(M, d, device=dev)                      # planes: 2 d halves = d floats
    xz = torch.randn(M, 2 * e, generator=g).to(dev)
    xc = torch.zeros(2, M, e, device=dev)
    xdbl = torch.zeros(2, M, r + 2 * N, device=dev)
    so = torch.zeros(M, e, device=dev)
    out = torch.zeros(M, d, device=dev)
    sws = torch.empty(lib.pope_vim_scan_workspace_bytes(B, L, e), dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    fp = C.c_void_p(flag.data_ptr()) if x3 else None
    P = _lib.ptr
    dirs = k.dir

    def linear_planes(a, wp, c, m, n, kk):
        return lambda: _lib.check(lib.pope_linear_planes_f32(P(a), wp, None, P(c), None, m, n, kk, 0, None, None, fp, None), "linear")

    def linear_prec(a, wf, c, m, n, kk):
        return lambda: _lib.check(lib.pope_linear_f32(P(a), wf, None, P(c), m, n, kk, 0, None, None, prec, fp, None), "linear")

    ops = {"add_rmsnorm": lambda: _lib.check(lib.pope_vim_add_rmsnorm_f32(P(hid), P(res), P(res), k.norm_w, None if x3 else P(op),
                                                                          P(op) if x3 else None, M, d, 1e-5, 1, 0, fp, None), "norm"),
           "in_proj": linear_planes(op, k.in_proj_wp, xz, M, 2 * e, d) if x3 else linear_prec(op, k.in_proj_w, xz, M, 2 * e, d),
           "conv1d_silu": lambda: _lib.check(lib.pope_vim_conv1d_silu_f32(P(xz), 2 * e, dirs, B, L, e, P(xc), None), "conv"),
           "x_proj_fwd": linear_prec(xc[0], k.dir[0].x_proj_w, xdbl[0], M, r + 2 * N, e),
           "x_proj_bwd": linear_prec(xc[1], k.dir[1].x_proj_w, xdbl[1], M, r + 2 * N, e),
           "scan": lambda: _lib.check(lib.pope_vim_scan_f32(P(xc), C.c_void_p(xz.data_ptr() + 4 * e), 2 * e, P(xdbl), dirs, B, L, e, r,
                                                            None if x3 else P(so), P(so) if x3 else None, P(sws), sws.numel(), fp, None), "scan"),
           "out_proj": linear_planes(so, k.out_proj_wp, out, M, d, e) if x3 else linear_prec(so, k.out_proj_w, out, M, d, e)}
    # realistic operands for the scan and its producers: one pass in model order before anything is timed
    for name in ("add_rmsnorm", "in_proj", "conv1d_silu", "x_proj_fwd", "x_proj_bwd", "scan", "out_proj"):
        ops[name]()
    torch.cuda.synchronize()
    floor_bytes = 4 * (5 * M * e + 2 * M * (r + 2 * N))
    return ops, floor_bytes


def eager_forward(sd, cfg, x):
    """The specification in eager torch on the device (fp32): what PyTorch-ROCm can do without a scan kernel."""
    d, depth = cfg["embed_dim"], cfg["depth"]
    e, r = 2 * d, -(-d // 16)
    tok = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=cfg["stride"]).flatten(2).transpose(1, 2)
    mid = tok.shape[1] // 2
    tok = torch.cat((tok[:, :mid], sd["cls_token"].expand(x.shape[0], -1, -1), tok[:, mid:]), dim=1) + sd["pos_embed"]
    hidden, residual = tok, None

    def rms(v, w):
        return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + 1e-5) * w

    def direction(xx, z, p, sfx, a_name, d_name):
        L = xx.shape[1]
        xp = F.pad(xx, (0, 0, 3, 0))
        wc = sd[p + f"conv1d{sfx}.weight"][:, 0]
        xc = F.silu(sd[p + f"conv1d{sfx}.bias"] + sum(wc[:, k] * xp[:, k:k + L] for k in range(4)))
        dbc = xc @ sd[p + f"x_proj{sfx}.weight"].t()
        delta = F.softplus(dbc[..., :r] @ sd[p + f"dt_proj{sfx}.weight"].t() + sd[p + f"dt_proj{sfx}.bias"])
        A = -torch.exp(sd[p + a_name])
        h = xx.new_zeros(xx.shape[0], e, N)
        ys = []
        for t in range(L):
            dl = delta[:, t, :, None]
            h = torch.exp(dl * A) * h + (dl * xc[:, t, :, None]) * dbc[:, t, None, r:r + N]
            ys.append((h * dbc[:, t, None, r + N:]).sum(-1) + sd[p + d_name] * xc[:, t])
        return torch.stack(ys, dim=1) * F.silu(z)

    for i in range(depth):
        p = f"layers.{i}.mixer."
        residual = hidden if residual is None else hidden + residual
        u = rms(residual, sd[f"layers.{i}.norm.weight"])
        xz = u @ sd[p + "in_proj.weight"].t()
        xx, z = xz[..., :e], xz[..., e:]
        o = direction(xx, z, p, "", "A_log", "D") + direction(xx.flip(1), z.flip(1), p, "_b", "A_b_log", "D_b").flip(1)
        hidden = (o / 2) @ sd[p + "out_proj.weight"].t()
    feat = rms((hidden + residual)[:, mid], sd["norm_f.weight"])
    return feat @ sd["head.weight"].t() + sd["head.bias"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vim_times.json"))
    ap.add_argument("--batches", default="2,48")
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vim_time.py measures on the GPU: no device found")
    case = synth.vim_case("small_s8")
    cfg, sd = case["cfg"], case["state_dict"]
    result = {"model": "vim_small_patch16_stride8_224 (L = 730, D = 384, E = 768, 24 layers)", "runs": []}
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 3, 224, 224, generator=g).cuda()
        eager_ms, eager_out = None, None
        if not args.no_eager:
            with torch.no_grad():
                eager_out = eager_forward(sd_dev, cfg, x)      # warm-up (and the comparison below)
                eager_ms = event_ms(lambda: eager_forward(sd_dev, cfg, x), warmup=0, reps=1)
        for precision in ("f16x3", "f32"):
            model = vim.VisionMamba(**{**vim._FACTORY_SETTINGS, **cfg}, precision=precision)
            model.load_state_dict(sd, strict=True)
            model = model.cuda()
            out = model(x)
            total = event_ms(lambda: model(x), warmup=2, reps=10)
            ops, floor_bytes = layer_ops(model, B, precision)
            per_op = {name: event_ms(fn) for name, fn in ops.items()}
            layer = sum(per_op.values())
            run = {"B": B, "precision": precision, "forward_ms": total, "layer_ops_ms": per_op, "layer_ms": layer,
                   "layers_ms": layer * cfg["depth"], "remainder_ms": total - layer * cfg["depth"],
                   "scan_fraction_of_layer": per_op["scan"] / layer, "scan_floor_bytes": floor_bytes,
                   "scan_floor_ms": floor_bytes / HBM_BYTES_PER_S * 1e3,
                   "scan_over_floor": per_op["scan"] / (floor_bytes / HBM_BYTES_PER_S * 1e3), "overflow_events": model.overflow_events}
            if eager_out is not None:
                run["eager_forward_ms"] = eager_ms
                run["max_abs_diff_to_eager"] = float((out - eager_out).abs().max())
            result["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
