"""Writes tests/golden/eapp_trunk.npz: the reference's own ResBlock_Custom(2, 32, 64) (model.py:88-130) on the CPU, fixed seed — the
fixture of model.ResBlockCustomFused (tests/test_gpu_eapp_trunk.py, tests/test_eapp_trunk_host.py).
  conv_res.weight/.bias, conv_ws.weight/.bias, conv.weight/.bias   the block's parameters (fp32)
  x    [2,32,12,20]  input: unit normal plus a per-channel offset of about -1, so that most GroupNorm shifts (-mean * rstd) are positive and
                     relu(shift) != 0: the case in which normalising a padded zero, instead of leaving it zero, shows in the border ring
  y32  [2,64,12,20]  the reference block's fp32 output
  y64  [2,64,12,20]  the same module in .double() on x.double()
Needs the reference checkout (oracle.import_reference); the tests read only the .npz.
usage: python tools/make_eapp_trunk_golden.py [out.npz]"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.import_reference import load_reference_model  # noqa: E402


def main(out):
    ref = load_reference_model()
    torch.manual_seed(20)
    block = ref.ResBlock_Custom(2, 32, 64).eval()
    g = torch.Generator().manual_seed(21)
    offset = -1.0 + 0.5 * torch.randn(32, generator=g)
    x = torch.randn(2, 32, 12, 20, generator=g) + offset.view(1, -1, 1, 1)
    with torch.no_grad():
        y32 = block(x)
        y64 = copy.deepcopy(block).double()(x.double())
    shifts = -x.mean(dim=(2, 3)) / x.var(dim=(2, 3), unbiased=False).add(1e-5).sqrt()   # 32 groups of one channel each
    assert (shifts > 0).float().mean().item() >= 0.75, "the offset should make most shifts positive"
    data = {k: v.detach().numpy() for k, v in block.state_dict().items()}
    data.update(x=x.numpy(), y32=y32.numpy(), y64=y64.numpy())
    np.savez_compressed(out, **data)
    e32 = (y32.double() - y64).abs().max().item()
    print(f"wrote {out}: {os.path.getsize(out)} bytes, max|y64| = {y64.abs().max().item():.3f}, reference fp32 error = {e32:.3e}, "
          f"positive shifts: {(shifts > 0).sum().item()} of {shifts.numel()}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "eapp_trunk.npz"))
