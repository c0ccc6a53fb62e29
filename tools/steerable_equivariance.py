"""ESCNNSteerableNetwork at angles that are not quarter turns: measured, CPU, fp64: python tools/steerable_equivariance.py

A smooth, radially windowed 65 x 65 image is rotated bilinearly about its centre by 10, 22.5 and 45 degrees (and by 90 as a check of
the rotation's sense against torch.rot90); the network (steerable.yaml: 16 fields, k = 7, 3 layers; eval mode, running statistics
= the statistics of the unrotated image) is evaluated on both.  Printed per seed and angle: the error of the first output vector's
angle against "turned by the same angle", and |v(rho x)| / |v(x)|.  The table goes into DESIGN.md next to the "exact for quarter
turns" statement.  --fields / --layers shrink the network for a quick look."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd.images.canonicalization_networks.steerable_networks import FieldNorm


def smooth_image(C: int, H: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(C, 1, H + 12, H + 12, generator=g, dtype=torch.float64)
    t = torch.arange(-6, 7, dtype=torch.float64)
    w = torch.exp(-t * t / 8.0)
    w = w / w.sum()
    x = F.conv2d(x, (w[:, None] * w[None, :])[None, None]).reshape(1, C, H, H)
    c = torch.arange(H, dtype=torch.float64) - (H - 1) / 2
    r = torch.sqrt(c[:, None] ** 2 + c[None, :] ** 2)
    return 10.0 * x * torch.clamp((H / 2 - 6 - r) / 6, 0, 1)


def rotate(x: torch.Tensor, deg: float) -> torch.Tensor:
    """Bilinear rotation about the centre in the sense of torch.rot90(x, 1, (-2, -1)) for deg = 90."""
    t = math.radians(deg)
    theta = torch.tensor([[[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0]]], dtype=x.dtype)
    grid = F.affine_grid(theta, list(x.shape), align_corners=True)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=16)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--kernel-size", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=3)
    args = ap.parse_args()
    print(f"{args.fields} fields, k = {args.kernel_size}, {args.layers} layers, 65 x 65, fp64")
    print("seed  angle   vector angle error [deg]   |v(rot x)| / |v(x)|")
    for seed in range(args.seeds):
        torch.manual_seed(seed)
        net = ea.ESCNNSteerableNetwork((3, 65, 65), args.fields, args.kernel_size, "rotation", args.layers).double()
        x = smooth_image(3, 65, 100 + seed)
        assert (rotate(x, 90.0) - torch.rot90(x, 1, (-2, -1))).abs().max() < 1e-9 * x.abs().max()
        with torch.no_grad():
            for m in net.block:
                if isinstance(m, FieldNorm):
                    m.momentum = 1.0
            net.train()
            net(x)
            net.eval()
            v = torch.view_as_complex(net(x)[0, 0].contiguous())
            for deg in (10.0, 22.5, 45.0, 90.0):
                vr = torch.view_as_complex(net(rotate(x, deg))[0, 0].contiguous())
                err = math.degrees(float(torch.angle(vr / v))) - deg
                err = (err + 180.0) % 360.0 - 180.0
                print(f"{seed:4d}  {deg:5.1f}   {err:+24.3f}   {float(vr.abs() / v.abs()):19.4f}")


if __name__ == "__main__":
    main()
