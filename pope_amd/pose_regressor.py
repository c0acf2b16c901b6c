"""The fork's learned pose head, `pose/model.py:Mkpts_Reg_Model`, on HIP (pose_regressor.hip): matched keypoints of a pair ->
(pred_trans [3], pred_rot [3, 3]).  Inference only, fp32 throughout, no torch fallback.

`Mkpts_Reg_Model(num_sample, mode)` keeps the reference constructor, its 78 state-dict keys (the unused template layer
`transformerlayer.*` included, so a reference checkpoint loads with strict=True) and the semantics of its forward: torch's
encoder is built with batch_first=False, so the B pairs of one call are read as ONE sequence and attention runs across
them, separately per sample slot — pair b's result depends on the other pairs of the call.  That is kept on purpose.
The notebooks evaluate one pair per call (`unsqueeze(0)`), which is what `regress_pose_batch` does for every pair of a batch
(attention groups of one), straight from the matcher's compacted device buffers.

Sampling (`pose/utils.py:collate_fn(num_sample)` runs before the module): a pair with MORE than num_sample matches is
sampled, any other pair (count == num_sample included) is zero-padded.  Two samplers:

* `sample_index` [B, S] int32, host-chosen.  `reference_sample_indices` replays the reference's `random.sample` sequence.
* the device sampler (default).  Definition, restated by `device_sample_indices` in numpy:
      key(i) = splitmix64(seed ^ ((i + 1) * 0xD1B54A32D192ED03 mod 2^64)),   i in [0, count)
      splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB;
                     return x ^ x >> 31                                       (all mod 2^64)
      slot j takes the match with the j-th smallest (key, i), j in [0, S)
  — a uniform ordered sample without replacement, like `random.sample`; it depends on the pair's own seed and count only.
"""
import ctypes as C
import random

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import check, on_device_of, require_cuda, stream_of

MODES = {"matrix": (0, 9), "quat": (1, 4), "6d": (2, 6)}     # mode -> (POPE_ROT_*, rotation_head width)
MAX_GROUP = 64
ROW_CHUNK = 8              # pairs a weight element of mlp.0 / mlp.3 is applied to per read (pose_regressor.hip CH)
MIN_MATCHES = 5            # pairs points_io.save_pair_points skips
COLLATE_SEED = 20231223    # pose/utils.py:109
_M64 = (1 << 64) - 1


class Mkpts_Reg_Model(nn.Module):
    """pose/model.py:43-114.  The torch submodules only hold the parameters under the reference's names; forward runs on HIP."""

    def __init__(self, num_sample: int, mode: str = "matrix"):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        self.num_sample, self.mode = int(num_sample), mode
        self.pts_size, self.N_freqs, self.inner_size = 2, 9, 32
        d = 2 * self.pts_size * (2 * self.N_freqs + 1)
        self.transformerlayer = nn.TransformerEncoderLayer(d_model=d, nhead=2)
        self.transformer = nn.TransformerEncoder(encoder_layer=self.transformerlayer, num_layers=4, enable_nested_tensor=False)
        self.translation_head = nn.Linear(self.inner_size, 3)
        self.rotation_head = nn.Linear(self.inner_size, MODES[mode][1])
        S = self.num_sample
        widths = [S * d, S * (2 * self.N_freqs + 1), S, 256, 128, 64, self.inner_size, self.inner_size]
        drops = [0.5, 0.2, 0.2, 0.1, 0.1, 0.1, 0.1]
        layers = []
        for i, p in enumerate(drops):
            layers += [nn.Linear(widths[i], widths[i + 1]), nn.LeakyReLU(), nn.Dropout(p=p)]
        self.mlp = nn.Sequential(*layers)
        self.eval()
        self._ws = None
        self._slots = None
        self._struct = None      # (key, struct, keep)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("Mkpts_Reg_Model runs inference only (dropout is not implemented): keep it in eval()")
        return super().train(False)

    def _weights(self):
        if self._slots is None:
            self._slots = _lib.param_slots(self)
        key = _lib.slots_key(self._slots)
        if self._struct is None or self._struct[0] != key:
            keep, w = [], _lib.PoseRegressorWeights()
            p = lambda t: _lib.param_ptr(t, keep, "Mkpts_Reg_Model")  # noqa: E731
            w.num_sample, w.mode = self.num_sample, MODES[self.mode][0]
            for i, layer in enumerate(self.transformer.layers):
                lw = w.layers[i]
                a = layer.self_attn
                for name, t in (("in_proj_w", a.in_proj_weight), ("in_proj_b", a.in_proj_bias), ("out_proj_w", a.out_proj.weight),
                                ("out_proj_b", a.out_proj.bias), ("linear1_w", layer.linear1.weight), ("linear1_b", layer.linear1.bias),
                                ("linear2_w", layer.linear2.weight), ("linear2_b", layer.linear2.bias), ("norm1_w", layer.norm1.weight),
                                ("norm1_b", layer.norm1.bias), ("norm2_w", layer.norm2.weight), ("norm2_b", layer.norm2.bias)):
                    setattr(lw, name, p(t))
            for i in range(7):
                w.mlp_w[i], w.mlp_b[i] = p(self.mlp[3 * i].weight), p(self.mlp[3 * i].bias)
            w.trans_w, w.trans_b = p(self.translation_head.weight), p(self.translation_head.bias)
            w.rot_w, w.rot_b = p(self.rotation_head.weight), p(self.rotation_head.bias)
            self._struct = (key, w, keep)
        return self._struct[1]

    def _dense(self, batch_mkpts0, batch_mkpts1, who):
        for t in (batch_mkpts0, batch_mkpts1):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who} expects torch tensors")
            require_cuda(t, who)
            if t.dtype != torch.float32:
                raise TypeError(f"{who} expects float32 keypoints")
        if batch_mkpts0.dim() != 3 or batch_mkpts0.shape != batch_mkpts1.shape or batch_mkpts0.shape[2] != 2:
            raise ValueError(f"{who}: batch_mkpts0 / batch_mkpts1 must both be [B, num_sample, 2]")
        if batch_mkpts0.shape[1] != self.num_sample:
            raise ValueError(f"{who}: {batch_mkpts0.shape[1]} sample rows, the model was built for num_sample = {self.num_sample}")
        if batch_mkpts0.shape[0] > MAX_GROUP:
            raise NotImplementedError(f"{who}: the B pairs of a call form one attention group; groups above {MAX_GROUP} are not implemented")
        if batch_mkpts0.shape[0] == 0:
            raise ValueError(f"{who}: empty batch")
        return batch_mkpts0.contiguous(), batch_mkpts1.contiguous()

    @torch.no_grad()
    def forward(self, batch_mkpts0, batch_mkpts1):
        """[B, num_sample, 2] x 2 -> (pred_trans [B, 3], pred_rot [B, 3, 3]); the B pairs are one attention group (B <= 64)."""
        if self.training:
            raise NotImplementedError("Mkpts_Reg_Model runs inference only")
        k0, k1 = self._dense(batch_mkpts0, batch_mkpts1, "Mkpts_Reg_Model.forward")
        out = _run(self, "forward", k0.shape[0], k0.shape[0], dense=(k0, k1))
        return out["t"], out["R"]

    @torch.no_grad()
    def taps(self, batch_mkpts0, batch_mkpts1, stage):
        """Test entry: X [B, S, 76] after the embedding (stage 'embedding') or after encoder layer 4 ('encoder')."""
        k0, k1 = self._dense(batch_mkpts0, batch_mkpts1, "Mkpts_Reg_Model.taps")
        return _run(self, stage, k0.shape[0], k0.shape[0], dense=(k0, k1))["x"]


def _run(model, stage, B, G, dense=None, compact=None, sample_index=None, seeds=None):
    lib = _lib.lib()
    S = model.num_sample
    src = dense[0] if dense else compact[0]
    dev = src.device
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d0, d1 = (p(dense[0]), p(dense[1])) if dense else (None, None)
    k0 = k1 = counts = None
    M = 0
    if compact:
        M = int(compact[0].shape[0])
        if M:
            k0, k1 = p(compact[0]), p(compact[1])
        counts = p(compact[2])
    status = torch.empty(B, dtype=torch.int32, device=dev)
    head = (d0, d1, k0, k1, counts, p(sample_index), p(seeds))
    with on_device_of(src):
        if stage == "embedding":
            x = torch.empty(B, S, 76, dtype=torch.float32, device=dev)
            index = torch.empty(B, S, dtype=torch.int32, device=dev)
            check(lib.pope_pose_regressor_embedding_f32(*head, B, S, M, p(x), p(index), p(status), stream_of(dev)),
                  "pope_pose_regressor_embedding_f32")
            return {"x": x, "index": index, "status": status}
        w = model._weights()
        if stage == "encoder":
            x = torch.empty(B, S, 76, dtype=torch.float32, device=dev)
            index = torch.empty(B, S, dtype=torch.int32, device=dev)
            check(lib.pope_pose_regressor_encoder_f32(C.byref(w), *head, B, S, G, M, p(x), p(index), p(status), stream_of(dev)),
                  "pope_pose_regressor_encoder_f32")
            return {"x": x, "index": index, "status": status}
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        need = lib.pope_pose_regressor_workspace_bytes(B, S)
        ws = _lib.grow_workspace(model, need, dev)
        check(lib.pope_pose_regressor_forward_f32(C.byref(w), *head, B, S, G, M, p(t), p(R), p(status), p(ws), ws.numel(), stream_of(dev)),
              "pope_pose_regressor_forward_f32")
    return {"R": R, "t": t, "status": status}


def compact_inputs(who, S, kpts0, kpts1, counts, seed, sample_index):
    """The checked device form of the pipeline inputs (see `regress_pose_batch`): kpts0, kpts1 [M, 2] fp32, counts [B] int32,
    sample_index [B, S] int32 or None, seeds [B] int64."""
    for t in (kpts0, kpts1):
        require_cuda(t, who)
        if t.dtype != torch.float32:
            raise TypeError(f"{who} expects float32 match coordinates")
    dev = kpts0.device
    kpts0, kpts1 = kpts0.contiguous(), kpts1.contiguous()
    M = int(kpts0.shape[0])
    if kpts0.shape != (M, 2) or kpts1.shape != (M, 2):
        raise ValueError("kpts0 / kpts1 must both be [M, 2]")
    counts = torch.as_tensor(counts)
    if not counts.is_cuda and counts.numel() and int(counts.min()) < 0:     # host counts are checked for free; device counts by the
        raise ValueError(f"{who}: negative match count")                  # kernel (status -1)
    counts = counts.to(device=dev, dtype=torch.int32).contiguous()
    B = int(counts.numel())
    if B == 0:
        raise ValueError(f"{who}: no pairs")
    if sample_index is not None:
        sample_index = torch.as_tensor(sample_index).to(device=dev, dtype=torch.int32).contiguous()
        if sample_index.shape != (B, S):
            raise ValueError(f"sample_index must be [B, num_sample] = [{B}, {S}]")
    if torch.is_tensor(seed):
        seeds = seed.to(device=dev, dtype=torch.int64).contiguous()
        if seeds.shape != (B,):
            raise ValueError("seed must be one integer or a [B] tensor")
    else:
        s = int(seed) & _M64
        seeds = torch.full((B,), s - (1 << 64) if s >> 63 else s, dtype=torch.int64, device=dev)
    return kpts0, kpts1, counts, sample_index, seeds


@torch.no_grad()
def regress_pose_batch(model, kpts0, kpts1, counts, seed=0, sample_index=None, stage="forward"):
    """The pipeline form: every pair on its own (an attention group of one), from the matcher's compacted device buffers.

    kpts0, kpts1 [M, 2] fp32 CUDA with the matches of pair b contiguous and the pairs in order, counts [B] int32 (the contract
    of `estimate_pose_batch`).  A pair with more than num_sample matches is sampled by `sample_index` [B, num_sample] int32 when
    given, else by the device sampler with `seed` (one integer for all pairs, or [B] int64); any other pair is zero-padded.
    Returns device tensors R [B, 3, 3], t [B, 3], status [B] int32 (0 ok; -1 refused: a negative count here or before it, or
    counts beyond M; -2 sample_index outside [0, count): zeros for such a pair).  No host synchronisation.
    `stage` 'embedding' / 'encoder' stop early (tests): {x [B, S, 76], index [B, S], status}."""
    if not isinstance(model, Mkpts_Reg_Model):
        raise TypeError("regress_pose_batch expects a pope_amd Mkpts_Reg_Model")
    if model.training:
        raise NotImplementedError("Mkpts_Reg_Model runs inference only")
    kpts0, kpts1, counts, sample_index, seeds = compact_inputs("regress_pose_batch", model.num_sample, kpts0, kpts1, counts, seed,
                                                               sample_index)
    B = int(counts.numel())
    return _run(model, stage, B, 1, compact=(kpts0, kpts1, counts), sample_index=sample_index, seeds=seeds)


def reference_sample_indices(counts, num_sample, rng=None):
    """`pose/utils.py:collate_fn(num_sample)` replayed on the host: Python's `random` seeded with 20231223 once, its state
    carried across pairs; a pair with more than num_sample matches draws `random.sample(range(count), num_sample)` TWICE —
    the reference samples `mkpts0` and then `mkpts1` with a draw each — any other pair draws nothing.  Returns int32
    [B, 2, num_sample]: [:, 0] the rows `mkpts0` keeps, [:, 1] those of `mkpts1` (identity and -1 padding for unsampled pairs).
    Pass `[:, 0]` as `sample_index` to keep both point sets on the rows the reference keeps of `mkpts0`.
    `rng`: a `random.Random` to continue from (default: a fresh one with the reference's seed)."""
    rng = rng or random.Random(COLLATE_SEED)
    out = np.full((len(counts), 2, num_sample), -1, np.int32)
    for b, c in enumerate(int(c) for c in counts):
        if c > num_sample:
            for k in range(2):
                out[b, k] = rng.sample(range(c), num_sample)
        else:
            out[b, :, :c] = np.arange(c, dtype=np.int32)
    return out


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def device_sample_indices(count, num_sample, seed=0):
    """numpy restatement of the device sampler (module docstring): the match per slot, int32 [num_sample]; identity and -1
    padding when count <= num_sample."""
    count = int(count)
    if count <= num_sample:
        out = np.full(num_sample, -1, np.int32)
        out[:max(count, 0)] = np.arange(max(count, 0), dtype=np.int32)
        return out
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64)
        keys = _splitmix64(np.uint64(int(seed) & _M64) ^ ((i + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)))
    order = np.lexsort((i, keys))          # by key, ties by index
    return order[:num_sample].astype(np.int32)
