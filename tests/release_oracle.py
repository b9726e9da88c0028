"""CPU restatement of the public HiFi-GAN release's Generator.forward (jik876/hifi-gan
models.py), written from its published definition; the oracle of test_release_host.py
and test_gpu_release.py.  Not a test module.

    x = conv_pre(mel)
    per stage i:  x = ups_i(leaky_relu(x, 0.1));  x = mean_j resblock_{i,j}(x)
        ResBlock1:  for m: x = convs2_m(lrelu(convs1_m(lrelu(x, 0.1)), 0.1)) + x
        ResBlock2:  for m: x = convs_m(lrelu(x, 0.1)) + x
    wav = tanh(conv_post(leaky_relu(x)))          # F.leaky_relu's default slope, 0.01

`cfg` carries the constructor lists plus `resblock` ("1" / "2", default "1") and
`final_lrelu_slope` (default 0.1, the reference's); with those defaults the op sequence
is that of oracle.hifigan_torch.generator_forward, bit for bit (asserted by
test_release_host.py before anything relies on this file).
"""
import torch
import torch.nn.functional as F


def block_forward(sd, pre, x, kr, dils, resblock):
    """One ResBlock1 / ResBlock2 with parameters `pre`.convs*; sd in x's dtype."""
    for m, d in enumerate(dils):
        if resblock == "2":
            xt = F.conv1d(F.leaky_relu(x, 0.1), sd[f"{pre}.convs.{m}.weight"],
                          sd[f"{pre}.convs.{m}.bias"], 1, (kr * d - d) // 2, d, 1)
        else:
            xt = F.conv1d(F.leaky_relu(x, 0.1), sd[f"{pre}.convs1.{m}.weight"],
                          sd[f"{pre}.convs1.{m}.bias"], 1, (kr * d - d) // 2, d, 1)
            xt = F.conv1d(F.leaky_relu(xt, 0.1), sd[f"{pre}.convs2.{m}.weight"],
                          sd[f"{pre}.convs2.{m}.bias"], 1, (kr - 1) // 2, 1, 1)
        x = x + xt
    return x


@torch.no_grad()
def release_forward(sd, cfg, mel, dtype=torch.float32):
    """mel [B, n_mels, T] -> wav [B, 1, L] in `dtype` (float32 or float64)."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    resblock = str(getattr(cfg, "resblock", "1"))
    post_slope = float(getattr(cfg, "final_lrelu_slope", 0.1))
    x = F.conv1d(torch.as_tensor(mel).to(dtype), sd["conv_pre.weight"], sd["conv_pre.bias"],
                 1, 3, 1, 1)
    n_res = len(cfg.resblock_kernel_sizes)
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], u, (k - u) // 2,
                               0, 1, 1)
        out = None
        for j, (kr, dils) in enumerate(zip(cfg.resblock_kernel_sizes,
                                           cfg.resblock_dilation_sizes)):
            xr = block_forward(sd, f"mrfs.{i}.resblocks.{j}", x, kr, dils, resblock)
            out = xr if out is None else out + xr
        x = out / n_res
    x = F.leaky_relu(x, post_slope)
    return torch.tanh(F.conv1d(x, sd["conv_post.weight"], sd["conv_post.bias"], 1, 3, 1, 1))


def scaled(sd, scale):
    """Every parameter times `scale` (the suite's weight-scale axis)."""
    return {k: v * scale for k, v in sd.items()}
