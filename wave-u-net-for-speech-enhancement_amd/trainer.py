"""train-step driver, selectable as the reference's trainer plugin

    "trainer": {"module": "wave-u-net-for-speech-enhancement_amd.trainer", "main": "Trainer", "epochs": ..., ...}

Same constructor as the reference's Trainer (/root/reference/trainer/trainer.py:13-25, called from train.py:41-49)
and the same `.train()` entry (train.py:51), covering the hot loop (trainer/trainer.py:27-43, base_trainer.py:187-197) and, opt-in,
a validation epoch scored on the device (below: SI-SDR improvement and, opt-in, STOI); TensorBoard and the host metric PESQ are out of
scope.
Differences from the reference loop, all on the f2 list:
  * one process per GPU: launched under torchrun (RANK / WORLD_SIZE / LOCAL_RANK in the environment) the constructor joins the
    process group itself (backend "nccl" = RCCL on a GPU box, "gloo" without one), pins the process to its GPU, re-wraps the
    incoming DataLoader with a DistributedSampler (train.py:15-21 builds it without one; the reference's batch_size is the
    GLOBAL batch that nn.DataParallel splits, base_trainer.py:26-27, so each rank loads batch_size / world_size items) and
    attaches the RCCL gradient all-reduce to the model instead of nn.DataParallel;
  * host->device copies are non_blocking from pinned memory (train.py:20 sets pin_memory but copies synchronously);
  * the loss is accumulated on the device and read back once per epoch (trainer.py:40 syncs every step);
  * after a few eager steps the whole step - forward, loss, backward, Adam (optim.FusedAdam with its device-side step counter) - is
    captured once in a hipGraph (torch.cuda.CUDAGraph) on static input buffers and replayed: ~230 kernel launches become one graph
    launch per step (default on one GPU with FusedAdam; `"graph": false` in the trainer config or WUNET_GRAPH=0 keeps eager launches;
    hyper-parameters that change every step - a per-step LR schedule - make it fall back to eager by itself, unless the optimiser
    reads its lr from device memory: `"device_lr": true` in the trainer config / FusedAdam(device_lr=True) keeps the one graph);
  * `"max_grad_norm": <float>` in the trainer config: gradient clipping by the global norm inside the fused step (optim.FusedAdam);
    `trainer.lr_scheduler` (None by default): its .step() is called after every optimiser step;
  * validation, strictly opt-in: with `"validation": {"metric": "si_sdr", "interval": N, "find_max": true, "custom": {"sample_length":
    16384}}` in the trainer config and a validation loader (batch 1 items `(mixture, clean, name)`, trainer/trainer.py:58-78), every N
    epochs rank 0 enhances each recording with inference.enhance in eval mode and scores the mean SI-SDR improvement in dB over the noisy
    input (metrics.si_sdr_improvement) - accumulated on the device, one device->host read per validation epoch.  The score is appended
    to `validation_scores`, compared with `best_score` as base_trainer.py:149-157 does, and a best one writes best_model.tar
    (base_trainer.py:118-120).  Every module's training flag (a frozen BatchNorm layer included) is restored afterwards, so a captured
    step graph stays valid.  Without the "metric" key the loader stays unused, as in earlier versions of this trainer;
  * `"validation": {"custom": {"margin": m, "fade": f, "window": "hann"}}` enhances with overlapped, cross-faded chunks and
    `"validation": {"recordings_per_pass": N}` enhances N recordings per pass in shared slabs (inference.py: enhance / enhance_many);
    the score, the one device->host read and the restored flags are the same.  Without these keys nothing changes;
  * `"validation": {"custom": {"sample_rate": 48000, "model_rate": 16000}}`: validation files at another rate than the network's.
    Every recording is resampled to "model_rate" on the device, enhanced, and resampled back to its own rate and length
    (inference.py: enhance(sample_rate=, model_rate=)); SI-SDR and STOI score at the files' rate, "sample_rate".  Without "model_rate",
    or with the two equal, nothing changes;
  * STOI, the first half of the reference's score (STOI + PESQ') / 2 (trainer/trainer.py:128-143), on the device: beside "metric":
    "si_sdr" the optional key `"stoi": "report"` also appends (mean STOI of the noisy recordings, mean STOI of the enhanced ones) to
    `validation_stoi` every validation epoch and leaves the score alone; `"stoi": "score"` makes the mean STOI of the enhanced
    recordings the epoch's score (`validation_scores` holds it, "find_max" applies as in the reference).  metrics.stoi at
    `"custom": {"sample_rate": 16000}` (the reference hard-codes 16 kHz); still one device->host read per validation epoch.
    `"stoi_extended": true` beside "stoi" makes both calls ESTOI (metrics.stoi(extended=True)); it needs the "stoi" key and a bool;
  * BSS Eval SDR, the score Wave-U-Net results are reported in (metrics.sdr: mir_eval's bss_eval_sources for one source), on the
    device: beside "metric": "si_sdr" the optional key `"sdr": "report"` also appends (mean SDR of the noisy recordings, mean SDR of
    the enhanced ones) [dB] to `validation_sdr` every validation epoch and leaves the score alone; `"sdr": "score"` makes the mean
    SDR of the enhanced recordings the epoch's score.  `"sdr_filter_length": n` (default 512) sets the forgiven filter's taps.  The
    recordings of a pass ("recordings_per_pass") are scored in one call, ragged, through `lengths`; with "model_rate" the score is
    at the files' rate.  Still one device->host read per validation epoch.  "stoi": "score" and "sdr": "score" together raise;
  * checkpoints keep the reference's names and keys (base_trainer.py:83-124) so either side can resume; only rank 0 writes.
"""
import os
from pathlib import Path

import torch
import torch.distributed as dist

from . import _lib
from .optim import FusedAdam
from .parallel import GradSync

GRAPH_WARMUP_STEPS = 3
# A captured step graph is given up for eager launches when MAX_RECAPTURES graphs IN A ROW did not earn their capture back: a graph
# earns REPLAY_CREDIT_S per replay (what a replay saves over the eager step when the loop synchronises: host launch jitter, 5.27 vs
# 5.5 ms median at the BASELINE size; back to back the two are level) and costs the measured wall time of its capture + instantiate;
# fewer than MIN_REPLAYS replays never count as earned.  A schedule that changes lr / betas / eps every step - or every 3 or 20 steps -
# therefore ends on eager launches after three captures, a per-epoch scheduler over long epochs keeps its graph.
MAX_RECAPTURES = 3
MIN_REPLAYS = 16
REPLAY_CREDIT_S = 0.25e-3
SDR_MAX_FILTER = _lib.CONSTANTS["WUNET_BSS_MAX_FILTER"]         # the longest forgiven filter of wunet_bss_sdr_forward


class Trainer:
    def __init__(self, config, resume, model, loss_function, optimizer, train_dataloader, validation_dataloader=None):
        env_world = int(os.environ.get("WORLD_SIZE", "1"))
        self._own_pg = False
        if env_world > 1 and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl" if torch.cuda.is_available() else "gloo")
            self._own_pg = True
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if torch.cuda.is_available():
            self.device = torch.device("cuda", local_rank)
            torch.cuda.set_device(self.device)
        else:
            self.device = torch.device("cpu")
        self.model = model.to(self.device)
        self.loss_function = loss_function
        self.optimizer = optimizer
        fused = isinstance(optimizer, FusedAdam)
        tcfg = config["trainer"]
        # "max_grad_norm" / "device_lr": options of the fused step (optim.FusedAdam); another optimiser cannot honour them
        for key in ("max_grad_norm", "device_lr"):
            if tcfg.get(key) is None:
                continue
            if not fused:
                raise ValueError(f'trainer config "{key}" needs optim.FusedAdam / FusedAdamW (got {type(optimizer).__name__}): '
                                 "it is applied inside the fused step")
            if key == "max_grad_norm" and not float(tcfg[key]) > 0.0:
                raise ValueError(f'trainer config "max_grad_norm" must be > 0 (got {tcfg[key]}); leave it out to train without clipping')
            setattr(optimizer, key, bool(tcfg[key]) if key == "device_lr" else float(tcfg[key]))
        # "native_rccl": the bucket all-reduces through the library's own RCCL entry (wunet_comm_*, capturable in the step graph)
        # instead of torch.distributed's process group; default: torch.distributed (measured on hardware only at world size 1 so far)
        native = bool(tcfg.get("native_rccl", os.environ.get("WUNET_NATIVE_RCCL", "0") not in ("", "0"))) and self.device.type == "cuda"
        if self.world > 1:
            from .parallel import NativeComm
            self.model.grad_sync = GradSync(scale_in_optimizer=fused, comm=NativeComm() if native else None)
            if fused:
                optimizer.grad_scale = 1.0 / self.world
        self.train_data_loader = self._shard_loader(train_dataloader)
        self.validation_data_loader = validation_dataloader      # used only with "validation": {"metric": "si_sdr", ...} (below)
        vcfg = tcfg.get("validation") or {}
        self.validation_metric = vcfg.get("metric")
        if self.validation_metric not in (None, "si_sdr"):
            raise ValueError(f'trainer config "validation.metric" must be "si_sdr" (got {self.validation_metric!r}); STOI is the key '
                             '"validation.stoi" beside it, PESQ is a host metric and out of scope')
        self.validation_interval = int(vcfg.get("interval", 0)) if self.validation_metric and validation_dataloader is not None else 0
        self.validation_find_max = bool(vcfg.get("find_max", True))
        self.validation_sample_length = int((vcfg.get("custom") or {}).get("sample_length", 16384))
        # overlapped chunks (inference.py: margin / fade / window) and several recordings per pass (inference.enhance_many), both opt-in
        custom = vcfg.get("custom") or {}
        self.validation_overlap = {key: custom[key] for key in ("margin", "fade", "window") if key in custom}
        if self.validation_overlap:
            from .inference import chunk_hop
            try:
                chunk_hop(self.validation_sample_length, **self.validation_overlap)
            except (ValueError, TypeError) as e:
                raise ValueError(f'trainer config "validation.custom": {e}') from None
        self.validation_recordings_per_pass = vcfg.get("recordings_per_pass")
        n_pass = self.validation_recordings_per_pass
        if n_pass is not None and (isinstance(n_pass, bool) or not isinstance(n_pass, int) or n_pass < 1):
            raise ValueError(f'trainer config "validation.recordings_per_pass" must be an integer >= 1 (got {n_pass!r}); leave it out to '
                             "enhance one recording at a time")
        self.validation_scores = []   # one mean SI-SDR improvement [dB] per validation epoch (the mean enhanced STOI with "stoi": "score")
        self.validation_stoi_mode = vcfg.get("stoi")
        if self.validation_stoi_mode not in (None, "report", "score"):
            raise ValueError(f'trainer config "validation.stoi" must be "report" or "score" (got {self.validation_stoi_mode!r})')
        if self.validation_stoi_mode is not None and self.validation_metric != "si_sdr":
            raise ValueError('trainer config "validation.stoi" needs "validation.metric": "si_sdr" beside it')
        self.validation_stoi_extended = vcfg.get("stoi_extended", False)
        if not isinstance(self.validation_stoi_extended, bool):
            raise ValueError(f'trainer config "validation.stoi_extended" must be true or false (got {self.validation_stoi_extended!r})')
        if "stoi_extended" in vcfg and self.validation_stoi_mode is None:
            raise ValueError('trainer config "validation.stoi_extended" needs "validation.stoi": "report" or "score" beside it')
        # "sdr": BSS Eval SDR (metrics.sdr) beside the SI-SDR improvement, reported or as the score; "sdr_filter_length": its taps
        self.validation_sdr_mode = vcfg.get("sdr")
        if self.validation_sdr_mode not in (None, "report", "score"):
            raise ValueError(f'trainer config "validation.sdr" must be "report" or "score" (got {self.validation_sdr_mode!r})')
        if self.validation_sdr_mode is not None and self.validation_metric != "si_sdr":
            raise ValueError('trainer config "validation.sdr" needs "validation.metric": "si_sdr" beside it')
        if self.validation_sdr_mode == "score" and self.validation_stoi_mode == "score":
            raise ValueError('trainer config "validation.stoi": "score" and "validation.sdr": "score" together: an epoch has one score')
        n_taps = vcfg.get("sdr_filter_length", 512)
        if isinstance(n_taps, bool) or not isinstance(n_taps, int) or not 1 <= n_taps <= SDR_MAX_FILTER:
            raise ValueError(f'trainer config "validation.sdr_filter_length" must be an integer in [1, {SDR_MAX_FILTER}] (got {n_taps!r})')
        if "sdr_filter_length" in vcfg and self.validation_sdr_mode is None:
            raise ValueError('trainer config "validation.sdr_filter_length" needs "validation.sdr": "report" or "score" beside it')
        self.validation_sdr_filter_length = n_taps
        self.validation_sdr = []      # with "validation.sdr": (mean SDR noisy, mean SDR enhanced) [dB] per validation epoch
        self.validation_sample_rate = int((vcfg.get("custom") or {}).get("sample_rate", 16000))
        # "custom.model_rate": the rate the network runs at when the validation files ("custom.sample_rate") are at another one - the
        # recordings are resampled to it, enhanced and resampled back on the device (inference.py); the scores stay at the files' rate
        self.validation_rates = {}
        if "model_rate" in custom:
            from .inference import _other_rate
            try:
                _other_rate(custom.get("sample_rate", 16000), custom["model_rate"])
            except ValueError as e:
                raise ValueError(f'trainer config "validation.custom": {e}') from None
            if custom["model_rate"] != self.validation_sample_rate:
                self.validation_rates = {"sample_rate": self.validation_sample_rate, "model_rate": int(custom["model_rate"])}
        self.validation_stoi = []     # with "validation.stoi": (mean STOI noisy, mean STOI enhanced) per validation epoch
        self.epochs = tcfg["epochs"]
        self.save_checkpoint_interval = tcfg.get("save_checkpoint_interval", 0)
        # default ON where it can be used (one GPU, or the native RCCL entry; fused Adam): the replay is as fast as the eager
        # launches back to back and a loop that synchronises every step (trainer/trainer.py:40 `loss.item()`) loses the host's launch
        # jitter (profiles/r4_graph_vs_eager.txt).  "graph": false / WUNET_GRAPH=0 turns it off.
        self.use_graph = bool(tcfg.get("graph", os.environ.get("WUNET_GRAPH", "1") not in ("", "0")))
        if self.use_graph and not (fused and self.device.type == "cuda" and (self.world == 1 or native)):
            # (torch.distributed's collectives stay outside a captured graph: their eager path overlaps them with the backward already;
            #  the native RCCL entry enqueues on the captured streams and is replayed with the step)
            self.use_graph = False
        if self.use_graph:
            optimizer.device_step = True
        self._graph = None
        self._graph_sig = None
        self._graph_bn = None          # the BatchNorm modes of the live graph (_bn_signature)
        self._static = None
        self._eager_steps = 0
        self._recaptures = 0          # consecutive graphs, dropped for a changed lr / betas / eps, that did not earn their capture back
        self._replays = 0
        self._capture_s = 0.0         # wall time of the live graph's capture
        self.captures = 0             # step graphs captured so far
        self.lr_scheduler = None      # set by the caller: .step() after every optimiser step (eager or replay)
        self.start_epoch = 1
        self.best_score = float("-inf") if self.validation_find_max or not self.validation_interval else float("inf")
        root = Path(os.path.expanduser(config.get("root_dir", "."))).absolute() / config.get("experiment_name", "exp")
        self.checkpoints_dir = root / "checkpoints"
        self.epoch_losses = []
        if resume:
            self._resume_checkpoint()

    # ---- data: every rank its own shard of each global batch (DataParallel's split, base_trainer.py:26-27)
    def _shard_loader(self, loader):
        if self.world == 1 or loader is None:
            return loader
        from torch.utils.data import DataLoader
        from torch.utils.data.distributed import DistributedSampler
        if isinstance(getattr(loader, "sampler", None), DistributedSampler):
            return loader
        if not isinstance(loader, DataLoader):
            raise TypeError("Trainer under torchrun needs a torch DataLoader (or one that already carries a DistributedSampler) "
                            "to shard the data; got " + type(loader).__name__)
        if loader.batch_size is None or loader.batch_size % self.world != 0:
            raise ValueError(f"batch_size={loader.batch_size} (the global batch, as nn.DataParallel would split it) must be a "
                             f"multiple of the world size {self.world}")
        shuffle = isinstance(loader.sampler, torch.utils.data.RandomSampler)
        # the reference's loader (train.py:15-21) keeps a ragged last batch: so does every rank here (the sampler pads the
        # dataset to equal per-rank counts instead of dropping items), and the loader's own options travel along
        sampler = DistributedSampler(loader.dataset, num_replicas=self.world, rank=self.rank, shuffle=shuffle, drop_last=False)
        extra = {}
        if loader.num_workers > 0:
            extra = dict(persistent_workers=loader.persistent_workers, prefetch_factor=loader.prefetch_factor)
        return DataLoader(loader.dataset, batch_size=loader.batch_size // self.world, sampler=sampler,
                          num_workers=loader.num_workers, pin_memory=loader.pin_memory, drop_last=loader.drop_last,
                          collate_fn=loader.collate_fn, worker_init_fn=loader.worker_init_fn, generator=loader.generator,
                          timeout=loader.timeout, **extra)

    # ---- checkpoints: reference layout (base_trainer.py:62-124)
    def _resume_checkpoint(self):
        path = self.checkpoints_dir / "latest_model.tar"
        assert path.exists(), f"{path} does not exist, can not load latest checkpoint."
        ckpt = torch.load(path.as_posix(), map_location=self.device)
        self.start_epoch = ckpt["epoch"] + 1
        self.best_score = ckpt["best_score"]
        self.optimizer.load_state_dict(ckpt["optimizer"])
        self.model.load_state_dict(ckpt["model"])

    def _save_checkpoint(self, epoch, is_best=False):
        if self.rank != 0:
            return
        self.checkpoints_dir.mkdir(parents=True, exist_ok=True)
        state = {"epoch": epoch, "best_score": self.best_score, "optimizer": self.optimizer.state_dict(),
                 "model": {k: v.cpu() for k, v in self.model.state_dict().items()}}
        torch.save(state, (self.checkpoints_dir / "latest_model.tar").as_posix())
        torch.save(state["model"], (self.checkpoints_dir / f"model_{str(epoch).zfill(4)}.pth").as_posix())
        if is_best:                                      # base_trainer.py:118-120
            torch.save(state, (self.checkpoints_dir / "best_model.tar").as_posix())

    # ---- validation (trainer/trainer.py:58-78 without the host metrics): mean SI-SDR improvement over the recordings, on the device
    def _is_best(self, score):
        """base_trainer.py:149-157."""
        if (score >= self.best_score) if self.validation_find_max else (score <= self.best_score):
            self.best_score = score
            return True
        return False

    @torch.no_grad()
    def _validation_epoch(self, epoch):
        from . import metrics
        from .inference import enhance, enhance_many
        model = getattr(self.model, "module", self.model)
        engine = getattr(model, "_engine_override", None)
        modes = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        gains, stois = [], []
        fs = self.validation_sample_rate
        per_pass = self.validation_recordings_per_pass

        def flush(held):
            many = {"sample_rates": self.validation_rates["sample_rate"], "model_rate": self.validation_rates["model_rate"]} if self.validation_rates else {}
            outs = enhance_many(model, [mix for mix, _ in held], self.validation_sample_length, **self.validation_overlap, **many)
            return [(mix, cl, out) for (mix, cl), out in zip(held, outs)]

        def passes():
            """(mixture, clean, enhanced) per recording, in the loader's order; with "recordings_per_pass" the recordings of a pass share
            the slabs of one enhance_many call."""
            held = []
            for mixture, clean, _name in self.validation_data_loader:
                if mixture.dim() != 3 or mixture.shape[0] != 1:
                    raise ValueError("Only support batch size is 1 in enhancement stage.")       # reference wording, trainer/trainer.py:64
                mixture = mixture.to(self.device, non_blocking=True)
                clean = clean.to(self.device, non_blocking=True)
                if per_pass is None:
                    yield mixture, clean, enhance(model, mixture, self.validation_sample_length, **self.validation_overlap, **self.validation_rates)
                    continue
                held.append((mixture, clean))
                if len(held) == per_pass:
                    yield from flush(held)
                    held = []
            if held:
                yield from flush(held)

        def sdr_of(group):
            """float32 [len(group), 2]: BSS Eval SDR of the noisy and of the enhanced recording of every (mixture, clean, enhanced) of
            `group` - the recordings of one pass, ragged, zero-padded to one slab and told apart by `lengths`: one call."""
            n, lens = len(group), [cl.shape[-1] for _, cl, _ in group]
            ref = torch.zeros(2, n, max(lens), dtype=torch.float32, device=self.device)
            est = torch.zeros_like(ref)
            for i, (mix, cl, enh) in enumerate(group):
                ref[:, i, :lens[i]] = cl.reshape(-1)
                est[0, i, :lens[i]] = mix.reshape(-1)
                est[1, i, :lens[i]] = enh.reshape(-1)
            lengths = torch.tensor(lens + lens, dtype=torch.int64).to(self.device, non_blocking=True)
            return metrics.sdr(ref, est, self.validation_sdr_filter_length, lengths=lengths, engine=engine).reshape(2, n).t()

        sdrs, group = [], []
        try:
            for mixture, clean, enhanced in passes():
                gains.append(metrics.si_sdr_improvement(clean, mixture, enhanced, engine=engine))
                if self.validation_stoi_mode is not None:
                    ext = self.validation_stoi_extended
                    stois.append(torch.cat([metrics.stoi(clean, mixture, sample_rate=fs, engine=engine, extended=ext).reshape(-1),
                                            metrics.stoi(clean, enhanced, sample_rate=fs, engine=engine, extended=ext).reshape(-1)]))
                if self.validation_sdr_mode is not None:
                    group.append((mixture, clean, enhanced))
                    if len(group) == (per_pass or 1):
                        sdrs.append(sdr_of(group))
                        group = []
            if group:
                sdrs.append(sdr_of(group))
        finally:
            for m, was in modes:                         # exactly the flags of before: a frozen BatchNorm layer stays frozen
                m.training = was
        if not gains:
            raise ValueError("validation: the validation loader yielded no recording")
        means = [torch.cat(gains).double().mean()]
        if stois:                                        # [recordings, 2]: noisy, enhanced
            means.extend(torch.stack(stois).double().mean(dim=0))
        if sdrs:                                         # [recordings, 2]: noisy, enhanced
            means.extend(torch.cat(sdrs).double().mean(dim=0))
        means = torch.stack(means).tolist()              # the only device->host read of the validation epoch
        score = means[0]
        if stois:
            self.validation_stoi.append((means[1], means[2]))
            if self.validation_stoi_mode == "score":
                score = means[2]
        if sdrs:
            self.validation_sdr.append((means[-2], means[-1]))
            if self.validation_sdr_mode == "score":
                score = means[-1]
        self.validation_scores.append(score)
        return score

    # ---- one step of the hot loop (trainer/trainer.py:34-38)
    def _eager_step(self, mixture, clean):
        self.optimizer.zero_grad(set_to_none=True)
        enhanced = self.model(mixture)
        loss = self.loss_function(clean, enhanced)
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def _capture(self, mixture, clean):
        """The step on static buffers, captured once (after the eager warm-up steps have created every lazily-built object:
        contexts, side stream, LDS attributes, optimiser state, device step counter)."""
        self._static = (mixture.clone(), clean.clone())
        self.optimizer.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            enhanced = self.model(self._static[0])
            loss = self.loss_function(self._static[1], enhanced)
            loss.backward()
            self.optimizer.step()               # (host side of step(): state["step"] += 1 happened once, here)
            self._static_loss = loss.detach()
        self._graph = graph
        self.captures += 1
        self._graph_sig = self.optimizer.hyper_signature()
        self._graph_bn = self._bn_signature()
        # capture does not execute: undo the host-side count of the captured call; every replay counts itself
        self.optimizer.advance_host_step(-1)

    def _bn_signature(self):
        """The BatchNorm modes the captured step was enqueued with (which layers are frozen, eval or training forward): part of
        the launches' arguments, so a change needs a new capture."""
        m = getattr(self.model, "module", self.model)
        frozen = getattr(m, "_bn_frozen", None)
        return (m.training, frozen() if frozen is not None else None)

    def _step(self, mixture, clean):
        loss = self._optimizer_step(mixture, clean)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        return loss

    def _optimizer_step(self, mixture, clean):
        if not self.use_graph:
            return self._eager_step(mixture, clean)
        if self._graph is not None and self._bn_signature() != self._graph_bn:
            # a BatchNorm module changed mode (frozen-BatchNorm fine-tuning): not a hyper-parameter change, capture again
            self._graph = None
            self._replays = 0
        if self._graph is not None and self.optimizer.hyper_signature() != self._graph_sig:
            # lr / betas / eps / grad_scale are kernel arguments of the captured Adam step: a scheduler, a manual decay or a
            # load_state_dict with another lr would be ignored by the replay - capture again with the new values.  A schedule that
            # changes them every step (or every few steps) would spend its time in capture + instantiate (far slower than eager):
            # after MAX_RECAPTURES graphs in a row that did not earn their capture back (see the constants), eager launches.
            self._graph = None
            earned = self._replays >= MIN_REPLAYS and self._replays * REPLAY_CREDIT_S >= self._capture_s
            self._recaptures = 0 if earned else self._recaptures + 1
            self._replays = 0
            if self._recaptures >= MAX_RECAPTURES:
                import warnings
                warnings.warn("Trainer: the optimiser's hyper-parameters change every few steps (a per-step LR schedule?); the captured "
                              "step graph would be rebuilt each time - falling back to eager launches (FusedAdam(device_lr=True) or "
                              '"device_lr": true in the trainer config keeps the graph under an lr schedule)', RuntimeWarning)
                self.use_graph = False
                self._fall_back_to_host_step()
                return self._eager_step(mixture, clean)
        if self._graph is None:
            if self._eager_steps < GRAPH_WARMUP_STEPS:
                self._eager_steps += 1
                return self._eager_step(mixture, clean)
            import time
            t0 = time.perf_counter()
            self._capture(mixture, clean)
            self._capture_s = time.perf_counter() - t0
        if mixture.shape != self._static[0].shape:          # a ragged last batch: eager (same kernels, same numbers)
            loss = self._eager_step(mixture, clean)
            return loss
        self._static[0].copy_(mixture, non_blocking=True)
        self._static[1].copy_(clean, non_blocking=True)
        self.optimizer.sync_device_hyper()                  # (device_lr: a changed lr reaches the device before the replay reads it)
        self._graph.replay()
        self._replays += 1
        self.optimizer.advance_host_step(1)
        return self._static_loss

    def _fall_back_to_host_step(self):
        """Eager from here on: the optimiser counts its steps on the host again (its state["step"] has been kept in step with the
        device counter by advance_host_step; the device counter is dropped and would be re-seeded if the graph ever came back)."""
        self.optimizer.device_step = False
        self.optimizer._dev = {}

    def _train_epoch(self, epoch):
        sampler = getattr(self.train_data_loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        loss_total = torch.zeros((), device=self.device)
        n = 0
        for mixture, clean, _name in self.train_data_loader:
            mixture = mixture.to(self.device, non_blocking=True)
            clean = clean.to(self.device, non_blocking=True)
            loss_total += self._step(mixture, clean)
            n += 1
        mean = (loss_total / max(n, 1)).item()          # the only device->host sync of the epoch
        self.epoch_losses.append(mean)
        return mean

    def train(self):
        for epoch in range(self.start_epoch, self.epochs + 1):
            self.model.train()
            self._train_epoch(epoch)
            if self.save_checkpoint_interval != 0 and epoch % self.save_checkpoint_interval == 0:
                self._save_checkpoint(epoch)
            if self.validation_interval != 0 and epoch % self.validation_interval == 0 and self.rank == 0:       # base_trainer.py:199-205
                if self._is_best(self._validation_epoch(epoch)):
                    self._save_checkpoint(epoch, is_best=True)
        if self._own_pg and dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
