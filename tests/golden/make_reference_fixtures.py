"""Record what the reference implementation itself computes, for the tests that check the package against it without it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_fixtures.py <reference checkout>

Imports the reference's model/unet_basic.py, model/loss.py, util/utils.py and train.py unmodified (shims/ first on sys.path for
the third-party imports it names) and writes, next to this file:

  port_ref_<case>.npz      its eval output, training output, loss, gradients and running statistics for the four shapes of
                           tests/test_oracle_golden.py::test_torch_port_equals_the_imported_reference (the 12-level shape keeps a
                           fixed, seeded sample of the gradients: the file size limit)
  init_reference.npz       its default initialisation under torch.manual_seed(0): the whole state of the 5-level / 8-channel net,
                           and a fixed, seeded sample of the 12-level / 24-channel one
  reference_main_epoch.npz the checkpoint its train.py:main writes after one epoch through this package's plugins (the config of
                           tests/test_reference_loader.py)
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
os.environ.setdefault("CUDA_VISIBLE_DEVICES", "-1")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1])
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "shims"), REF):
    sys.path.insert(0, p)

import numpy as np        # noqa: E402
import torch              # noqa: E402

from oracle import plan   # noqa: E402

PORT_CASES = [(3, 4, 2, 64, "mse"), (5, 8, 3, 512, "l1"), (4, 6, 2, 256, "smooth_l1"), (12, 24, 2, 4096, "mse")]
PORT_THREADS = 8                      # ATen's CPU reductions split by the thread count: recorded and compared under this one
GRAD_SAMPLE = 1 << 17                 # gradient entries kept of a net above that size (12 levels: 10.1 M)
INIT_SAMPLE = 1 << 16


def case_name(n, ci, B, T, loss_kind):
    return f"{n}x{ci}_B{B}_T{T}_{loss_kind}"


def sample_positions(size, k, seed):
    return np.sort(np.random.default_rng(seed).choice(size, k, replace=False))


def port_cases():
    from model.unet_basic import Model as RefModel
    from model import loss as ref_loss
    torch.set_num_threads(PORT_THREADS)
    for n, ci, B, T, loss_kind in PORT_CASES:
        sd_np = plan.golden_state(n, ci, seed=0)
        noisy_np, clean_np = plan.golden_batch(B, T, seed=0)
        noisy, clean = torch.from_numpy(noisy_np), torch.from_numpy(clean_np)
        model = RefModel(n_layers=n, channels_interval=ci)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()})
        crit = {"mse": ref_loss.mse_loss, "l1": ref_loss.l1_loss, "smooth_l1": torch.nn.SmoothL1Loss}[loss_kind]()
        model.eval()
        with torch.no_grad():
            out_eval = model(noisy).numpy().copy()
        model.train()
        out = model(noisy)
        loss = crit(clean, out)
        loss.backward()
        fx = {"meta": np.array([n, ci, B, T], np.int64), "threads": np.array(PORT_THREADS), "loss_kind": np.array(loss_kind), "torch_version": np.array(torch.__version__),
              "out_eval": out_eval, "out_train": out.detach().numpy(), "loss": np.array(loss.item(), np.float32)}
        grads = [p.grad.numpy().ravel() for _, p in model.named_parameters()]
        flat = np.concatenate(grads)
        fx["grad_norms"] = np.array([np.sqrt(np.sum(np.square(g.astype(np.float64)))) for g in grads])      # (no BLAS: thread-independent)
        if flat.size > GRAD_SAMPLE:
            fx["grad_positions"] = sample_positions(flat.size, GRAD_SAMPLE, 0)
            fx["grad_flat"] = flat[fx["grad_positions"]]
        else:
            fx["grad_flat"] = flat
        post = model.state_dict()
        for k in plan.buffer_names(n, ci):
            fx["buf/" + k] = post[k].numpy()
        path = os.path.join(HERE, "port_ref_" + case_name(n, ci, B, T, loss_kind) + ".npz")
        np.savez_compressed(path, **fx)
        print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


def init_states():
    from model.unet_basic import Model as RefModel
    torch.manual_seed(0)
    small = RefModel(n_layers=5, channels_interval=8).state_dict()
    torch.manual_seed(0)
    full = RefModel().state_dict()
    flat = torch.cat([v.reshape(-1).double() for v in full.values()]).numpy()
    fx = {"small_keys": np.array(list(small.keys())), "full_keys": np.array(list(full.keys())),
          "full_shapes": np.array([list(v.shape) + [0] * (3 - v.dim()) for v in full.values()], np.int64),
          "full_positions": sample_positions(flat.size, INIT_SAMPLE, 1)}
    fx["full_sample"] = flat[fx["full_positions"]]
    for k, v in small.items():
        fx["small/" + k] = v.numpy()
    path = os.path.join(HERE, "init_reference.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


def main_epoch():
    import test_reference_loader as t
    import train as ref_train
    with tempfile.TemporaryDirectory() as d:
        cfg = t.main_config(d)
        ref_train.main(cfg, resume=False)
        ck = torch.load(os.path.join(d, cfg["experiment_name"], "checkpoints", "latest_model.tar"))
    fx = {"epoch": np.array(ck["epoch"], np.int64), "keys": np.array(list(ck["model"].keys()))}
    for k, v in ck["model"].items():
        fx["model/" + k] = v.numpy()
    path = os.path.join(HERE, "reference_main_epoch.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    port_cases()
    init_states()
    main_epoch()
