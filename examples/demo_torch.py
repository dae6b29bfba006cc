#!/usr/bin/env python3
"""Register a batch of image pairs that already live on the GPU.

The images are torch CUDA tensors (here made on the device from a shifted
pattern); BatchRegistration reads them where they are and returns the motion
as a CUDA tensor, ordered with torch's current stream: no host copy on the way
in or out.

    python examples/demo_torch.py [--batch 64] [--size 128]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    import torch
    from opticalflow2d_amd import BatchRegistration
    B, n = a.batch, a.size
    dev = torch.device("cuda", 0)
    # a smooth pattern and B copies of it shifted along x by 0 .. 2 pixels
    x = torch.arange(n, device=dev, dtype=torch.float32)
    shift = torch.linspace(0.0, 2.0, B, device=dev).view(B, 1, 1)
    ref = torch.sin(x.view(n, 1) / 9.0) * torch.cos(x.view(1, n) / 7.0)        # [n, n], shared
    mov = torch.sin((x.view(1, n, 1) + shift) / 9.0) * torch.cos(x.view(1, 1, n) / 7.0)
    with BatchRegistration(B, (n, n), [200], 0, 0.1, device=0) as b:
        b.register(ref, mov)                   # CUDA tensors: read in place
        motion = b.motion_device()             # [B, n, n, 2] float32 on the GPU
        warped = b.warp(mov)                   # [B, n, n] float32 on the GPU
        iters = b.iterations()[:, -1]
    ux = motion[..., 0].mean(dim=(1, 2)).cpu()
    before = (mov - ref).abs().mean(dim=(1, 2)).cpu()
    after = (warped - ref).abs().mean(dim=(1, 2)).cpu()
    print("pair  shift  iterations  mean u_x  |Imov - Iref|  |warped - Iref|")
    for k in range(B):
        print(f"{k:4d}  {float(shift[k]):5.2f}  {int(iters[k]):10d}  {float(ux[k]):8.3f}  "
              f"{float(before[k]):13.5f}  {float(after[k]):15.5f}")


if __name__ == "__main__":
    main()
