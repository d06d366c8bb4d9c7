"""CPU ORACLE (test infrastructure, NOT product code) for the Hybrid Demucs v3 path (`hdemucs_mmi`).

A from-scratch restatement of `HDemucs.forward` in eval mode (reference: demucs/hdemucs.py:689-794) for the reference's
default hyper-parameters (depth 6, channels 48, cac, hybrid, dconv_mode 1 with BLSTM + LocalState from layer 4,
GroupNorm(4) from layer 4), as plain functions over a state dict in float32 or float64.  Only `tests/`,
`__graft_entry__.smoke()` and `bench.py`'s `cpu_baseline` leg may import it.

Pinned by `tests/golden/hseg_*.npz` / `happly_*.npz`, produced by `tools/make_golden.py` from the imported reference
(float32 and float64 runs with this repo's synthetic weights); see tests/test_oracle_golden.py.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from .htdemucs_oracle import istft_from_cac, stft_cac

Tensor = torch.Tensor


def unfold(a: Tensor, kernel_size: int, stride: int) -> Tensor:
    """demucs/utils.py:20-35: frames of `kernel_size` every `stride`, right zero-padded so that F = ceil(T / stride)."""
    length = a.shape[-1]
    n_frames = math.ceil(length / stride)
    tgt = (n_frames - 1) * stride + kernel_size
    a = F.pad(a, (0, tgt - length))
    return a.unfold(-1, kernel_size, stride)                      # (..., F, K)


def lstm_direction(x: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, reverse: bool) -> Tensor:
    """One direction of one nn.LSTM layer, zero initial state; x (T, N, D) -> (T, N, H).  Gate order i, f, g, o."""
    T, N, _ = x.shape
    H = w_hh.shape[1]
    gx = x @ w_ih.t() + (b_ih + b_hh)                             # (T, N, 4H)
    h = x.new_zeros(N, H)
    c = x.new_zeros(N, H)
    out = x.new_empty(T, N, H)
    steps = range(T - 1, -1, -1) if reverse else range(T)
    for t in steps:
        g = gx[t] + h @ w_hh.t()
        i, f, gg, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return out


def blstm(sd: Dict[str, Tensor], p: str, x: Tensor) -> Tensor:
    """BLSTM(dim, layers=2, max_steps=200, skip=True) (demucs/demucs.py:20-67): (B, C, T) -> (B, C, T)."""
    B, C, T = x.shape
    y = x
    framed = T > 200
    width, stride = 200, 100
    if framed:
        frames = unfold(x, width, stride)                          # (B, C, F, width)
        nframes = frames.shape[2]
        x = frames.permute(0, 2, 1, 3).reshape(-1, C, width)
    x = x.permute(2, 0, 1)                                        # (T, N, C)
    for layer in range(2):
        fw = lstm_direction(x, sd[f"{p}.lstm.weight_ih_l{layer}"], sd[f"{p}.lstm.weight_hh_l{layer}"],
                            sd[f"{p}.lstm.bias_ih_l{layer}"], sd[f"{p}.lstm.bias_hh_l{layer}"], False)
        bw = lstm_direction(x, sd[f"{p}.lstm.weight_ih_l{layer}_reverse"], sd[f"{p}.lstm.weight_hh_l{layer}_reverse"],
                            sd[f"{p}.lstm.bias_ih_l{layer}_reverse"], sd[f"{p}.lstm.bias_hh_l{layer}_reverse"], True)
        x = torch.cat([fw, bw], dim=-1)
    x = F.linear(x, sd[f"{p}.linear.weight"], sd[f"{p}.linear.bias"]).permute(1, 2, 0)    # (N, C, T)
    if framed:
        x = restitch(x.reshape(B, -1, C, width), stride, T)
    return x + y


def restitch(fr: Tensor, stride: int, length: int) -> Tensor:
    """demucs/demucs.py:51-64: frames (B, F, C, width) -> (B, C, length).  Every frame drops stride // 2 columns on the sides it
    shares with a neighbour (the first keeps its start, the last its end); the kept parts are concatenated and cut."""
    nframes = fr.shape[1]
    limit = stride // 2
    parts = []
    for k in range(nframes):
        if k == 0:
            parts.append(fr[:, k, :, :-limit])
        elif k == nframes - 1:
            parts.append(fr[:, k, :, limit:])
        else:
            parts.append(fr[:, k, :, limit:-limit])
    return torch.cat(parts, -1)[..., :length]


def local_attention(q: Tensor, k: Tensor, content: Tensor, decay_logits: Tensor) -> Tensor:
    """The attention core of LocalState (demucs/demucs.py:196-214): q, k, content (B, heads, dh, T), decay_logits
    (B, heads, ndecay, T) -> (B, heads * dh, T).  score[key t, query s] = k_t . q_s / sqrt(dh) - |t - s| * sum_f (f + 1) *
    (sigmoid(d_f[s]) / 2) / sqrt(ndecay), the diagonal FILLED with -100 (not removed), softmax over the keys."""
    B, heads, dh, T = q.shape
    ndecay = decay_logits.shape[2]
    idx = torch.arange(T, dtype=q.dtype)
    delta = idx[:, None] - idx[None, :]                           # left index keys, right index queries
    dots = torch.einsum("bhct,bhcs->bhts", k, q) / dh ** 0.5
    decays = torch.arange(1, ndecay + 1, dtype=q.dtype)
    dq = torch.sigmoid(decay_logits) / 2
    kernel = -decays.view(-1, 1, 1) * delta.abs() / ndecay ** 0.5
    dots = dots + torch.einsum("fts,bhfs->bhts", kernel, dq)
    dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -100)
    w = torch.softmax(dots, dim=2)
    return torch.einsum("bhts,bhct->bhcs", w, content).reshape(B, -1, T)


def local_state(sd: Dict[str, Tensor], p: str, x: Tensor, heads: int = 4, ndecay: int = 4) -> Tensor:
    """LocalState(channels, heads=4, ndecay=4) (demucs/demucs.py:182-216): attention over keys t for every query s with
    a per-query decay penalty on |t - s| and the diagonal masked to -100."""
    B, C, T = x.shape
    q = F.conv1d(x, sd[f"{p}.query.weight"], sd[f"{p}.query.bias"]).view(B, heads, -1, T)
    k = F.conv1d(x, sd[f"{p}.key.weight"], sd[f"{p}.key.bias"]).view(B, heads, -1, T)
    dl = F.conv1d(x, sd[f"{p}.query_decay.weight"], sd[f"{p}.query_decay.bias"]).view(B, heads, ndecay, T)
    content = F.conv1d(x, sd[f"{p}.content.weight"], sd[f"{p}.content.bias"]).view(B, heads, -1, T)
    res = local_attention(q, k, content, dl)
    return x + F.conv1d(res, sd[f"{p}.proj.weight"], sd[f"{p}.proj.bias"])


def dconv(sd: Dict[str, Tensor], p: str, x: Tensor, lstm: bool, attn: bool, depth: int = 2) -> Tensor:
    """DConv residual branch (demucs/demucs.py:133-154) on (R, C, T) rows, optional BLSTM + LocalState between the
    GELU and the 1x1 (module indices shift accordingly)."""
    for d in range(depth):
        q = f"{p}.dconv.layers.{d}"
        dil = 2 ** d
        y = F.conv1d(x, sd[f"{q}.0.weight"], sd[f"{q}.0.bias"], dilation=dil, padding=dil)
        y = F.gelu(F.group_norm(y, 1, sd[f"{q}.1.weight"], sd[f"{q}.1.bias"], eps=1e-5))
        i = 3
        if lstm:
            y = blstm(sd, f"{q}.{i}", y)
            i += 1
        if attn:
            y = local_state(sd, f"{q}.{i}", y)
            i += 1
        y = F.conv1d(y, sd[f"{q}.{i}.weight"], sd[f"{q}.{i}.bias"])
        y = F.glu(F.group_norm(y, 1, sd[f"{q}.{i + 1}.weight"], sd[f"{q}.{i + 1}.bias"], eps=1e-5), dim=1)
        x = x + sd[f"{q}.{i + 3}.scale"][:, None] * y
    return x


def _gn(sd, p: str, x: Tensor, on: bool, groups: int = 4) -> Tensor:
    return F.group_norm(x, groups, sd[f"{p}.weight"], sd[f"{p}.bias"], eps=1e-5) if on else x


def enc_layer(sd, p: str, L: dict, x: Tensor, time_branch: bool, inject: Optional[Tensor] = None) -> Tensor:
    """HEncLayer.forward (demucs/hdemucs.py:123-157) for a frequency (4-D), merged-time (3-D) or time-branch layer."""
    freq = L["freq"] and not time_branch
    if not freq and x.dim() == 4:
        x = x.reshape(x.shape[0], -1, x.shape[-1])
    stri = L["stri"] if not time_branch else 4
    if not freq:
        le = x.shape[-1]
        if le % stri:
            x = F.pad(x, (0, stri - le % stri))
    pad = (L["ker"] // 4 if L["pad"] else 0) if not time_branch else 2
    if freq:
        y = F.conv2d(x, sd[f"{p}.conv.weight"], sd[f"{p}.conv.bias"], stride=(stri, 1), padding=(pad, 0))
    else:
        y = F.conv1d(x, sd[f"{p}.conv.weight"], sd[f"{p}.conv.bias"], stride=stri, padding=pad)
    if time_branch and L["tenc_empty"]:
        return y
    if inject is not None:
        y = y + (inject[:, :, None] if inject.dim() == 3 and y.dim() == 4 else inject)
    y = F.gelu(_gn(sd, f"{p}.norm1", y, L["norm"]))
    if freq:
        B, C, Fr, T = y.shape
        r = y.permute(0, 2, 1, 3).reshape(-1, C, T)
        y = dconv(sd, p, r, L["lstm"], L["attn"]).view(B, Fr, C, T).permute(0, 2, 1, 3)
        z = F.conv2d(y, sd[f"{p}.rewrite.weight"], sd[f"{p}.rewrite.bias"])
    else:
        y = dconv(sd, p, y, L["lstm"], L["attn"])
        z = F.conv1d(y, sd[f"{p}.rewrite.weight"], sd[f"{p}.rewrite.bias"])
    return F.glu(_gn(sd, f"{p}.norm2", z, L["norm"]), dim=1)


def dec_layer(sd, p: str, L: dict, x: Tensor, skip: Optional[Tensor], length: int, time_branch: bool, last: bool):
    """HDecLayer.forward (demucs/hdemucs.py:304-335); dconv_mode = 1 puts no DConv in the decoders.  Returns (z, pre)."""
    freq = L["freq"] and not time_branch
    empty = time_branch and L["tenc_empty"]
    if freq and x.dim() == 3:
        x = x.view(x.shape[0], L["chout_z"], -1, x.shape[-1])
    if not empty:
        x = x + skip
        if freq:
            y = F.conv2d(x, sd[f"{p}.rewrite.weight"], sd[f"{p}.rewrite.bias"], padding=1)
        else:
            y = F.conv1d(x, sd[f"{p}.rewrite.weight"], sd[f"{p}.rewrite.bias"], padding=1)
        y = F.glu(_gn(sd, f"{p}.norm1", y, L["norm"]), dim=1)
    else:
        y = x
    stri = L["stri"] if not time_branch else 4
    pad = (L["ker"] // 4 if L["pad"] else 0) if not time_branch else 2
    if freq:
        z = F.conv_transpose2d(y, sd[f"{p}.conv_tr.weight"], sd[f"{p}.conv_tr.bias"], stride=(stri, 1))
    else:
        z = F.conv_transpose1d(y, sd[f"{p}.conv_tr.weight"], sd[f"{p}.conv_tr.bias"], stride=stri)
    z = _gn(sd, f"{p}.norm2", z, L["norm"])
    if freq:
        if pad:
            z = z[..., pad:-pad, :]
    else:
        z = z[..., pad:pad + length]
    return (z if last else F.gelu(z)), y


def hdemucs_forward(sd: Dict[str, Tensor], mix: Tensor, plan: List[dict], n_sources: int = 4, taps: Optional[dict] = None) -> Tensor:
    """mix (B, 2, L), any L -> (B, S, 2, L).  `plan` = demucs_amd.hdemucs_weights.hdemucs_layer_plan(cfg)."""
    B, _, length = mix.shape
    S = n_sources
    mag = stft_cac(mix)                                            # hdemucs.py:693-695 (_spec + _magnitude, cac)
    if taps is not None: taps["stft"] = mag
    mean = mag.mean(dim=(1, 2, 3), keepdim=True)
    std = mag.std(dim=(1, 2, 3), keepdim=True)
    x = (mag - mean) / (1e-5 + std)
    meant = mix.mean(dim=(1, 2), keepdim=True)
    stdt = mix.std(dim=(1, 2), keepdim=True)
    xt = (mix - meant) / (1e-5 + stdt)
    saved, saved_t, lengths, lengths_t = [], [], [], []
    n_tenc = sum(1 for L in plan if L["has_tenc"])
    for idx, L in enumerate(plan):
        lengths.append(x.shape[-1])
        inject = None
        if idx < n_tenc:
            lengths_t.append(xt.shape[-1])
            xt = enc_layer(sd, f"tencoder.{idx}", L, xt, True)
            if taps is not None: taps[f"tenc{idx}"] = xt
            if not L["tenc_empty"]:
                saved_t.append(xt)
            else:
                inject = xt
        x = enc_layer(sd, f"encoder.{idx}", L, x, False, inject)
        if idx == 0 and taps is not None: taps["enc0_preemb"] = x
        if idx == 0:                                               # hdemucs.py:734-739
            emb = (sd["freq_emb.embedding.weight"] * 10.0).t()[None, :, :, None]
            x = x + 0.2 * emb
        if taps is not None: taps[f"enc{idx}"] = x
        saved.append(x)
    x = torch.zeros_like(x)
    xt = torch.zeros_like(x)
    depth = len(plan)
    offset = depth - n_tenc
    for j in range(depth):
        L = plan[depth - 1 - j]
        skip = saved.pop(-1)
        x, pre = dec_layer(sd, f"decoder.{j}", L, x, skip, lengths.pop(-1), False, last=j == depth - 1)
        if taps is not None: taps[f"dec{j}"] = x
        if j >= offset:
            length_t = lengths_t.pop(-1)
            if L["tenc_empty"]:
                xt, _ = dec_layer(sd, f"tdecoder.{j - offset}", L, pre[:, :, 0], None, length_t, True, last=False)
            else:
                xt, _ = dec_layer(sd, f"tdecoder.{j - offset}", L, xt, saved_t.pop(-1), length_t, True, last=j == depth - 1)
            if taps is not None: taps[f"tdec{j - offset}"] = xt
    Fq, T = x.shape[-2:]
    x = x.view(B, S, -1, Fq, T) * std[:, None] + mean[:, None]
    x = istft_from_cac(x, length)
    xt = xt.view(B, S, -1, length) * stdt[:, None] + meant[:, None]
    return xt + x


class OracleHDemucs:
    """Model object for `apply_oracle.apply_model`: no `valid_length`, any input length (like the reference's HDemucs)."""

    def __init__(self, sd_np: dict, cfg, dtype=torch.float32):
        from demucs_amd.hdemucs_weights import hdemucs_layer_plan
        self.sd = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in sd_np.items()}
        self.plan = hdemucs_layer_plan(cfg)
        self.dtype = dtype
        self.sources = list(cfg.sources)
        self.samplerate = cfg.samplerate
        self.audio_channels = cfg.audio_channels
        self.segment = cfg.segment

    def __call__(self, mix: Tensor) -> Tensor:
        with torch.no_grad():
            return hdemucs_forward(self.sd, mix.to(self.dtype), self.plan, len(self.sources))
