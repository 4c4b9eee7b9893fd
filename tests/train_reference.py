"""Test-side restatement of the restorer in train mode (the reference's mode 2): restorer/model.py:69-120 and
restorer/modules.py with every BatchNorm on batch statistics and the two Dropout(0.5) layers replaced by given masks
(voicefixer_amd.dropout.mask).  One segment at a time (batch 1, as the reference calls it), in any dtype; reuses the
eval oracle's GRU, conv and layout code.  torch's own batch_norm does the normalising, so a BatchNorm that sees one value
per channel raises the same ValueError as the reference."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle


def _bn(x, sd, p):
    return F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], training=True, eps=1e-5)


def denoiser(mel, sd, masks, p="denoiser"):
    """(1,1,T,128) -> mask (1,1,T,128); ``masks`` = (m0, m1), each (T, 512): 0 or 2."""
    m0, m1 = masks
    x = _bn(mel, sd, p + ".0")
    x = F.relu(F.linear(x, sd[p + ".1.weight"], sd[p + ".1.bias"]))
    x = _bn(x, sd, p + ".3")
    x = F.linear(x, sd[p + ".4.weight"], sd[p + ".4.bias"]) * m0
    x = F.relu(x)
    for g in (".7", ".8"):
        x = _bn(x, sd, p + g + ".bn")[:, 0]
        for layer in (0, 1):
            outs = []
            for suf, rev in (("", False), ("_reverse", True)):
                q = "%s%s.gru." % (p, g)
                outs.append(oracle._gru_dir(x, sd[q + "weight_ih_l%d%s" % (layer, suf)], sd[q + "weight_hh_l%d%s" % (layer, suf)],
                                            sd[q + "bias_ih_l%d%s" % (layer, suf)], sd[q + "bias_hh_l%d%s" % (layer, suf)], rev))
            x = torch.cat(outs, dim=-1)
        x = x[:, None]
    x = F.relu(_bn(x, sd, p + ".9"))
    x = F.linear(x, sd[p + ".11.weight"], sd[p + ".11.bias"]) * m1
    x = F.relu(_bn(x, sd, p + ".13"))
    return torch.sigmoid(F.linear(x, sd[p + ".15.weight"], sd[p + ".15.bias"]))


def conv_block_res(x, sd, p):
    origin = x
    x = F.conv2d(F.leaky_relu(_bn(x, sd, p + ".bn1"), 0.01), sd[p + ".conv1.weight"], padding=1)
    x = F.conv2d(F.leaky_relu(_bn(x, sd, p + ".bn2"), 0.01), sd[p + ".conv2.weight"], padding=1)
    if (p + ".shortcut.weight") in sd:
        return F.conv2d(origin, sd[p + ".shortcut.weight"], sd[p + ".shortcut.bias"]) + x
    return origin + x


def unet(x, sd, p="unet"):
    """model_kqq_bn.py:130-181 in train mode: (1,2,T,128) -> (1,1,T,128)."""
    T = x.shape[2]
    x = F.pad(x, pad=(0, 0, 0, int(np.ceil(T / 64)) * 64 - T))
    x = x[..., 0: x.shape[-1] - 1]
    skips = []
    for b in range(1, 7):
        for k in (1, 2, 3, 4):
            x = conv_block_res(x, sd, "%s.encoder_block%d.conv_block%d" % (p, b, k))
        skips.append(x)
        x = F.avg_pool2d(x, kernel_size=(2, 2))
    x = conv_block_res(x, sd, p + ".conv_block7")
    for b in range(1, 7):
        q = "%s.decoder_block%d" % (p, b)
        x = F.conv_transpose2d(F.relu(_bn(x, sd, q + ".bn1")), sd[q + ".conv1.weight"], stride=2)[:, :, 0:-1, :]
        x = torch.cat((x, skips[6 - b]), dim=1)
        for k in (2, 3, 4, 5):
            x = conv_block_res(x, sd, "%s.conv_block%d" % (q, k))
    x = conv_block_res(x, sd, p + ".after_conv_block1")
    x = F.conv2d(x, sd[p + ".after_conv2.weight"], sd[p + ".after_conv2.bias"])
    x = F.pad(x, pad=(0, 1))
    return x[:, :, 0:T, :]


def restorer_forward(mel, sd, masks):
    """Generator.forward (restorer/model.py:103-120) in train mode: mel (1,1,T,128) -> dict of "mask", "unet_out", "mel"
    (the restored log-mel)."""
    mask = denoiser(mel, sd, masks)
    x = oracle.to_log(mask * mel)
    unet_out = unet(torch.cat([oracle.to_log(mel), x], dim=1), sd)
    return {"mask": mask, "unet_out": unet_out, "mel": unet_out + x}


def masks_for(seed, segment, T, dtype=torch.float64):
    from voicefixer_amd import dropout
    return tuple(torch.from_numpy(dropout.mask(seed, segment, layer, T)).to(dtype) for layer in (0, 1))


def restore_segment(wav, voc_sd, res_sd, seed, segment=0, dtype=torch.float64):
    """One segment through front-end, train-mode restorer and vocoder (base.py:123-135 in mode 2), as
    oracle.restore_inmem does it for mode 0: numpy (n,) -> float numpy (1, n)."""
    w = torch.as_tensor(np.asarray(wav), dtype=dtype)
    cast = (lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()})
    voc, res = cast(oracle._canon(voc_sd)), cast(res_sd)
    mel = oracle.wav_to_mel(w[None], dtype)
    den = oracle.from_log(restorer_forward(mel, res, masks_for(seed, segment, mel.shape[2], dtype))["mel"])
    out = oracle.vocoder_forward(den, voc)
    peak = torch.max(torch.abs(out))
    if peak > 1.0:
        out = out / peak
    return oracle.trim_center(out, w.shape[0]).reshape(1, -1).numpy()
