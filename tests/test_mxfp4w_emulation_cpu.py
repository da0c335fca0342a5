"""An fp32 emulation of the stated MXFP4 linear semantics (exact element values, fp32 sum, SwiGLU and bias in fp32, one
rounding to T) over the case list of tests/test_gpu_mxfp4w.py, against the same float64 oracle and bound: the reference
arithmetic itself keeps the bound within EMULATION_WORST, the figure that file quotes, before any kernel is blamed."""
import numpy as np
import pytest
import torch

import test_gpu_mxfp4w as mc


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_fp32_emulation_meets_the_oracle_within_the_quoted_share_of_the_bound(built_lib, dt):
    worst = 0.0
    for m, n, k, bias, _, swiglu, _ in mc.CASES + [(17, 24, 64, 1, 0, 0, ""), (17, 24, 64, 0, 0, 1, "")]:
        x, ws, b, ref = mc.operands(m, n, k, bias, swiglu, dt)
        for _, _, d in ws:  # every element value is a value of T (the scale contract), so also of fp32
            assert np.array_equal(torch.from_numpy(d).to(mc.TORCH_DT[dt]).double().numpy(), d)
        xt = torch.from_numpy(x.astype(np.float32))
        v = xt @ torch.from_numpy(ws[0][2].astype(np.float32)).t()
        if swiglu:
            v = v / (1.0 + torch.exp(-v)) * (xt @ torch.from_numpy(ws[1][2].astype(np.float32)).t())
        if bias:
            v = v + torch.from_numpy(b.astype(np.float32))
        worst = max(worst, mc.ratio(v.to(mc.TORCH_DT[dt]).double().numpy(), ref, dt))
    assert worst <= mc.EMULATION_WORST, worst
