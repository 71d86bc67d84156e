"""Record ref_noise_12x24_B16.npz: the reference's own fp32 distance from exact, per gradient tensor, under every host thread count in
THREADS, for tests/test_gpu_parity.py::test_gemm_paths_match_reference (12 levels, 24 channels, batch 16 x 16384, smooth-L1,
golden_state(seed 0), golden_batch(seed 5)).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ref_noise.py

The reference's ATen CPU path (oracle/torch_port.py, bit-identical to the reference) splits its reductions by the number of threads it
runs on.  Recorded on one host: under 1-32 and 128 threads every tensor sits at most 2.04e-3 from the float64 arbiter; under 64 threads
the deep encoder BatchNorm gradients reach 7.0e-3 .. 1.05e-2 (encoder.9.main.1.bias 1.63e-3 at 16 threads, 9.49e-3 at 64; a factor of
up to 12 between rows on one tensor).  Another host's CPU kernels (ISA dispatch) move the figures by a few percent more.  The test
judges the HIP gradients against the worst of these and of the distance measured on its own host, and says so."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np    # noqa: E402
import torch          # noqa: E402

from oracle import plan, torch_port   # noqa: E402

THREADS = (1, 2, 4, 8, 16, 32, 64, 128)
n, ci, B, T = 12, 24, 16, 16384

if __name__ == "__main__":
    noisy, clean = plan.golden_batch(B, T, 5)
    t64 = torch_port.state_to_torch(plan.golden_state(n, ci, 0), dtype=torch.float64, requires_grad=True)
    o64 = torch_port.forward(t64, torch.from_numpy(noisy).double(), n, ci, True)
    torch_port.loss_value("smooth_l1", torch.from_numpy(clean).double(), o64).backward()
    names = plan.param_names(n, ci)
    rel = np.zeros((len(THREADS), len(names)))
    for i, nt in enumerate(THREADS):
        torch.set_num_threads(nt)
        tsd = torch_port.state_to_torch(plan.golden_state(n, ci, 0), requires_grad=True)
        out = torch_port.forward(tsd, torch.from_numpy(noisy), n, ci, True)
        torch_port.loss_value("smooth_l1", torch.from_numpy(clean), out).backward()
        for j, k in enumerate(names):
            arb = t64[k].grad
            rel[i, j] = ((tsd[k].grad.double() - arb).norm() / (arb.norm() + 1e-30)).item()
        print(f"{nt} threads: done", flush=True)
    np.savez_compressed(os.path.join(HERE, "ref_noise_12x24_B16.npz"), names=np.array(names), threads=np.array(THREADS), rel=rel,
                        meta=np.array([n, ci, B, T], np.int64), torch_version=np.array(torch.__version__))
