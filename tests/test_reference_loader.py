"""The drop-in boundary as the REFERENCE's own code drives it: its config loader (`util/utils.py:55-72
initialize_config`: import "module", take "main", call it with "args" unless pass_args is false) resolves the config strings of
INTEGRATION.md §1 to this package, the product Model is seed-for-seed identical to the reference's at construction (same 177 state_dict
entries, same default init), and the reference's `train.py:main` runs an epoch through the product's trainer / dataset / model plugins.
The reference does not travel with the package: what it produced is recorded under tests/golden/ (make_reference_fixtures.py writes
init_reference.npz and reference_main_epoch.npz; init_digest.npz pins the whole default init), and its loader and entry point are
restated here in the form the plugins see them."""
import importlib
import os

import numpy as np
import torch

from conftest import PKG_NAME, ROOT


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)


def initialize_config(module_cfg, pass_args=True):
    """The reference's config convention: the object named "main" in module "module", called with "args" when pass_args."""
    obj = getattr(importlib.import_module(module_cfg["module"]), module_cfg["main"])
    return obj(**module_cfg["args"]) if pass_args else obj


def reference_main(config, resume):
    """What the reference's train.py:main does with a config: seed torch and numpy, build the train / validation DataLoaders, the model,
    torch.optim.Adam, the loss and the trainer class from the config, and run trainer.train()."""
    torch.manual_seed(config["seed"])
    np.random.seed(config["seed"])
    dl = config["train_dataloader"]
    train_loader = torch.utils.data.DataLoader(dataset=initialize_config(config["train_dataset"]), batch_size=dl["batch_size"],
                                               num_workers=dl["num_workers"], shuffle=dl["shuffle"], pin_memory=dl["pin_memory"])
    valid_loader = torch.utils.data.DataLoader(dataset=initialize_config(config["validation_dataset"]), num_workers=1, batch_size=1)
    model = initialize_config(config["model"])
    optimizer = torch.optim.Adam(params=model.parameters(), lr=config["optimizer"]["lr"],
                                 betas=(config["optimizer"]["beta1"], config["optimizer"]["beta2"]))
    loss_function = initialize_config(config["loss_function"])
    trainer_class = initialize_config(config["trainer"], pass_args=False)
    trainer_class(config=config, resume=resume, model=model, loss_function=loss_function, optimizer=optimizer,
                  train_dataloader=train_loader, validation_dataloader=valid_loader).train()


def main_config(root_dir):
    """The one-epoch config of test_reference_train_py_runs_an_epoch_through_the_plugins (its checkpoint is recorded from the reference)."""
    return {
        "seed": 0, "root_dir": str(root_dir), "experiment_name": "ref_main",
        "train_dataset": {"module": PKG_NAME + ".dataset", "main": "Dataset", "args": {"n_items": 6, "sample_length": 64, "seed": 1}},
        "validation_dataset": {"module": PKG_NAME + ".dataset", "main": "Dataset", "args": {"n_items": 1, "sample_length": 64}},
        "train_dataloader": {"batch_size": 3, "num_workers": 0, "shuffle": False, "pin_memory": False},
        "model": {"module": "emu_plugins", "main": "Model", "args": {"n_layers": 2, "channels_interval": 4}},
        "optimizer": {"lr": 1e-3, "beta1": 0.9, "beta2": 0.999},
        "loss_function": {"module": "emu_plugins", "main": "mse_loss", "args": {}},
        "trainer": {"module": PKG_NAME + ".trainer", "main": "Trainer", "epochs": 1, "save_checkpoint_interval": 1},
    }


def _init_digest(state_dict):
    out = []
    for k, v in state_dict.items():
        a = v.detach().double().numpy().ravel()
        out.append([a.size, a.sum(), np.abs(a).sum(), a[0], a[-1]])
    return np.array(out, np.float64)


def test_default_init_matches_committed_digest(pkg):
    """torch.manual_seed(0); Model() -> the digest recorded from the reference's Model() under the same seed."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "init_digest.npz"))
    torch.manual_seed(0)
    m = pkg.Model()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["keys"]]
    assert sum(p.numel() for p in m.parameters()) == 10132802
    np.testing.assert_array_equal(_init_digest(sd), fx["digest"])


def test_default_init_is_seed_for_seed_the_references(pkg):
    """torch.manual_seed(0); Model(**kw) -> the reference's Model(**kw) under the same seed: the whole state of the 5-level / 8-channel
    net and a fixed, seeded sample of the 12-level / 24-channel one, bit for bit; its checkpoints load into the product's Model."""
    fx = _golden("init_reference")
    torch.manual_seed(0)
    ours = pkg.Model(n_layers=5, channels_interval=8)
    os_ = ours.state_dict()
    assert list(os_.keys()) == [str(k) for k in fx["small_keys"]]
    rs = {k: torch.from_numpy(fx["small/" + k]) for k in os_}
    for k in rs:
        assert rs[k].shape == os_[k].shape and torch.equal(rs[k], os_[k]), k
    ours.load_state_dict(rs)                  # reference checkpoints load
    torch.manual_seed(0)
    sd = pkg.Model().state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["full_keys"]]
    assert [list(v.shape) + [0] * (3 - v.dim()) for v in sd.values()] == fx["full_shapes"].tolist()
    flat = torch.cat([v.reshape(-1).double() for v in sd.values()]).numpy()
    np.testing.assert_array_equal(flat[fx["full_positions"]], fx["full_sample"])


def test_reference_initialize_config_resolves_the_integration_strings():
    """The config strings of INTEGRATION.md section 1 resolve through the reference's loader convention - as restated above
    (initialize_config), not through the reference's own util/utils.py, which does not travel with the package."""
    model = initialize_config({"module": PKG_NAME + ".model", "main": "Model", "args": {}})
    assert isinstance(model, torch.nn.Module) and model.n_layers == 12 and model.channels_interval == 24
    assert len(model.state_dict()) == 177
    small = initialize_config({"module": PKG_NAME + ".model", "main": "Model", "args": {"n_layers": 3, "channels_interval": 4}})
    assert small.n_layers == 3
    for name in ("mse_loss", "l1_loss", "smooth_l1_loss"):
        crit = initialize_config({"module": PKG_NAME + ".loss", "main": name, "args": {}})
        assert callable(crit)
    trainer_cls = initialize_config({"module": PKG_NAME + ".trainer", "main": "Trainer"}, pass_args=False)
    assert trainer_cls is importlib.import_module(PKG_NAME + ".trainer").Trainer
    ds = initialize_config({"module": PKG_NAME + ".dataset", "main": "Dataset", "args": {"n_items": 5, "sample_length": 64}})
    mix, clean, name = ds[0]
    assert mix.shape == (1, 64) and len(ds) == 5


def test_reference_train_py_runs_an_epoch_through_the_plugins(tmp_path):
    """train.py:main(config, resume) (restated above as reference_main): it builds the DataLoaders, torch.optim.Adam and calls our
    trainer plugin's .train() - with the model / loss plugins bound to the CPU emulator engine (tests/emu_plugins.py), since the
    product path has no CPU fallback.  Result == the checkpoint the reference's own train.py wrote from the same config
    (tests/golden/reference_main_epoch.npz) == the written-out loop of trainer/trainer.py:30-38.  What runs here is the restatement
    of train.py:main, not the reference's file; and the recorded checkpoint went through this package's trainer / dataset / model
    plugins too, so it pins the product as the reference's entry drove it - the independent check is the written-out loop."""
    cfg = main_config(tmp_path)
    reference_main(cfg, resume=False)
    ck = torch.load((tmp_path / "ref_main" / "checkpoints" / "latest_model.tar").as_posix())
    assert ck["epoch"] == 1 and len(ck["model"]) == 7 * 5 + 2
    fx = _golden("reference_main_epoch")
    assert int(fx["epoch"]) == ck["epoch"] and [str(k) for k in fx["keys"]] == list(ck["model"].keys())
    for k, v in ck["model"].items():
        assert torch.equal(v, torch.from_numpy(fx["model/" + k])), k
    # the same two steps written out (train.py:12-13 seeds, :29 model, :31-35 Adam; trainer/trainer.py:30-38)
    import emu_plugins
    torch.manual_seed(0)
    np.random.seed(0)
    ds = importlib.import_module(PKG_NAME + ".dataset").Dataset(n_items=6, sample_length=64, seed=1)
    m = emu_plugins.Model(n_layers=2, channels_interval=4)
    opt = torch.optim.Adam(params=m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    crit = emu_plugins.mse_loss()
    m.train()
    for mix, cl, _ in torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False):
        opt.zero_grad()
        crit(cl, m(mix)).backward()
        opt.step()
    for k, v in m.state_dict().items():
        assert torch.equal(v, ck["model"][k]), k
