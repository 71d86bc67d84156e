"""The case table of chunked enhancement with overlap (chunk_gather_kernel / chunk_overlap_add_kernel behind wunet_chunk_gather /
wunet_chunk_overlap_add, inference.enhance / enhance_many), shared by tests/test_chunks_emu.py (CPU emulator) and
tests/test_gpu_chunks.py (MI355X): what runs, on which tensors, and the checks against the float64 oracle of tests/chunks_ref.py.
`engine` None = the product's default engine.

The model of the arithmetic cases is a stub in eval mode, y[i][0][j] = a[j] x[i][0][j] + b[j] with fixed random a, b of L values: it
depends on the position inside the chunk, so a wrong offset shows, and any L is allowed.  The oracle gathers its own chunks (which must
equal what the model was given, bit for bit), pushes them through the same stub and overlap-adds in float64 with the same float32 ramp
and the same float32 1 - ramp.

The bar (derived, not measured).  Outside the cross-fades a sample is a copy: bit equality with y_k[m + j].  Inside, with w = ramp[j],
w' = fl(1 - w) (the oracle uses the same float32 w'), A = y_k[m + j], B = y_(k-1)[m + H + j], the kernel computes
fl(w A + fl(w' B)) - a product rounded once and one fused multiply-add - where the oracle has w A + w' B exactly:
    |out - ref| <= 2^-24 |w' B| + 2^-24 |w A + w' B| (1 + 2^-24)  <=  2^-23 (|w A| + |w' B|)
(three roundings of 2^-24 each when the build does not fuse, to first order; fusing only lowers it).  Every check prints the worst
ratio |out - ref| / bar before it asserts."""
import functools
import importlib

import numpy as np
import torch

import chunks_ref as R
from conftest import PKG_NAME

SENTINEL = 12345.0

# name: (L, m, f, recording lengths)
CASES = {
    "b": (64, 8, 16, (1, 16, 48, 49, 200)),      # T = 48: one chunk, T = 49: two - the boundary of the chunk count
    "c": (64, 0, 32, (200,)),                    # f = H: every sample after the first hop is in a cross-fade
    "d": (64, 12, 0, (200,)),                    # pure discard: bit equality everywhere, no ramp
    "e": (50, 3, 7, (123,)),                     # L % 4 != 0 (and the recording one float into a NaN-guarded array, below)
    "f": (64, 8, 16, (1, 37, 64, 200, 1000)),    # enhance_many, max_batch = 3: recordings straddle slabs
}
REAL = (16384, 2048, 2048, 50000)                # cases g, h (GPU): one real-size row, H = 10240, 5 chunks
WINDOWS = ("hann", "linear")


def inference():
    return importlib.import_module(PKG_NAME + ".inference")


def engine_or_default(engine):
    return engine if engine is not None else importlib.import_module(PKG_NAME + ".engine").default_engine()


def bit_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


class Stub(torch.nn.Module):
    """y = a x + b per position of the chunk (identity=True: y = x), in eval mode; keeps what it was given."""

    def __init__(self, L, identity=False, seed=7):
        super().__init__()
        rng = np.random.default_rng(seed)
        self.register_buffer("a", torch.from_numpy(rng.uniform(0.5, 1.5, L).astype(np.float32) * rng.choice([-1.0, 1.0], L).astype(np.float32)))
        self.register_buffer("b", torch.from_numpy(rng.uniform(-0.3, 0.3, L).astype(np.float32)))
        self.identity = identity
        self.seen = []
        self._engine_override = None
        self.eval()

    def forward(self, x):
        assert x.dim() == 3 and x.shape[1] == 1 and x.shape[2] == self.a.numel() and x.is_contiguous()
        self.seen.append(x.clone())
        return x.clone() if self.identity else x * self.a + self.b


class Recorder(torch.nn.Module):
    """Any model in eval mode, keeping its inputs and outputs (the oracle is then fed with the device's own chunk outputs)."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.seen, self.said = [], []
        self._engine_override = getattr(inner, "_engine_override", None)
        self.eval()

    def forward(self, x):
        y = self.inner(x)
        self.seen.append(x.clone())
        self.said.append(y.clone())
        return y


@functools.lru_cache(maxsize=None)
def recording(T, seed=0):
    """float32 [T] in [-1, 1) - built once, shared, never modified."""
    x = np.random.default_rng(1000 * seed + T).uniform(-1.0, 1.0, T).astype(np.float32)
    x.setflags(write=False)
    return x


def stub_outputs(stub, chunks_np):
    """The oracle's chunks through the stub's own arithmetic, on the host."""
    x = torch.from_numpy(chunks_np)
    return (x.clone() if stub.identity else x * stub.a.cpu() + stub.b.cpu()).numpy()


def check_against(ref, out, label):
    """The bar of this file's docstring on every sample of one recording; prints the worst ratio first."""
    o32 = out.detach().cpu().reshape(-1)
    o = o32.double().numpy()
    assert o.shape == ref["out"].shape, (label, o.shape, ref["out"].shape)
    assert np.isfinite(o).all(), f"{label}: NaN / Inf (or a sample never written)"
    faded = ref["faded"]
    d, bar = np.abs(o - ref["out"]), 2.0 ** -23 * (ref["wa"] + ref["wb"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.nan_to_num(d[faded] / bar[faded], nan=0.0, posinf=np.inf)
    core_ok = bit_equal(o32[torch.from_numpy(~faded)], torch.from_numpy(ref["copy"][~faded]))
    print(f"{label}: T {len(o)}  {int(faded.sum())} cross-faded samples, worst |out - ref| / bar {ratio.max() if ratio.size else 0.0:.3f}; "
          f"the other {int((~faded).sum())} bit-equal: {core_ok}")
    assert core_ok, f"{label}: a sample outside the cross-fades is not the chunk's own bits"
    assert (d[faded] <= bar[faded]).all(), (label, float(ratio.max()))


def reference_for(x, L, m, f, window, stub=None, said=None):
    """The oracle for one recording: from the stub (its own gather, the stub's arithmetic) or from recorded chunk outputs."""
    T = len(x)
    y = stub_outputs(stub, R.gather(x, L, m, f)) if said is None else said
    oa = R.overlap_add if T <= 4096 else R.overlap_add_fast
    return oa(np.ascontiguousarray(y, np.float32), T, L, m, f, R.ramp(f, window) if f else None)


def enhance_one(engine, device, x, L, m, f, window, model, **kw):
    mix = torch.from_numpy(np.array(x)).to(device).view(1, 1, -1)
    out = inference().enhance(model, mix, sample_length=L, margin=m, fade=f, window=window, engine=engine, **kw)
    assert out.shape == (1, 1, len(x)) and out.dtype == torch.float32
    return out


def check_stub_case(name, engine, device, window="hann", identity=False):
    """Cases b - e through inference.enhance with the stub: the gather equals the oracle's bit for bit, the output meets the bar."""
    L, m, f, lengths = CASES[name]
    for T in lengths:
        x = recording(T)
        stub = Stub(L, identity=identity).to(device)
        out = enhance_one(engine, device, x, L, m, f, window, stub)
        given = torch.cat(stub.seen).cpu()[:, 0]
        assert bit_equal(given, torch.from_numpy(R.gather(x, L, m, f))), f"case {name} T {T}: the gathered chunks differ from the oracle's"
        assert given.shape[0] == R.count(T, L, m, f)
        ref = reference_for(x, L, m, f, window, stub=stub)
        if T <= 4096:                                     # (the two forms of the oracle agree)
            fast = R.overlap_add_fast(stub_outputs(stub, R.gather(x, L, m, f)), T, L, m, f, R.ramp(f, window) if f else None)
            assert all(np.array_equal(ref[key], fast[key]) for key in ref)
        check_against(ref, out, f"case {name} T {T} {window}{' identity' if identity else ''}")
        if identity:
            # out equals the input: the bar with A = B = x, the core bit for bit
            xin = {"out": x.astype(np.float64), "faded": ref["faded"], "copy": x, "wa": ref["wa"], "wb": ref["wb"]}
            check_against(xin, out, f"case {name} T {T} {window} identity against the input")
        again = enhance_one(engine, device, x, L, m, f, window, Stub(L, identity=identity).to(device))
        assert bit_equal(out, again), f"case {name} T {T}: two runs differ"
    if name == "b":
        assert [R.count(T, L, m, f) for T in lengths] == [1, 1, 1, 2, 6]
    if name == "c":
        # (n = 6: every sample behind the first hop is in a cross-fade, up to the last chunk's tail [192, 200), which has no down-ramp)
        assert ref["faded"][32:192].all() and not ref["faded"][:32].any() and not ref["faded"][192:].any()
    if name == "d":
        assert not ref["faded"].any()


def guarded(x, device, offset=1, guard=float("nan"), tail=3):
    """x as a view `offset` floats into a buffer of guards (4-byte aligned only): (view, buffer)."""
    buf = torch.full((offset + len(x) + tail,), guard, dtype=torch.float32)
    buf[offset:offset + len(x)] = torch.from_numpy(np.array(x))
    buf = buf.to(device)
    return buf[offset:offset + len(x)], buf


def check_case_e_guards(engine, device):
    """Case e on the two entries themselves: the recording one float into a NaN-guarded flat array, the output one float into a buffer
    of sentinels.  No NaN comes out, both guards survive."""
    L, m, f, (T,) = CASES["e"]
    eng, inf = engine_or_default(engine), inference()
    x = recording(T)
    flat, fbuf = guarded(x, device)
    before = fbuf.clone()
    rows, recs, _ = inf.chunk_tables([T], L, m, f)
    n = rows.shape[0]
    chunks = torch.full((n, 1, L), float("nan"), device=device)
    eng.chunk_gather(flat, torch.from_numpy(rows).to(device), chunks)
    assert bit_equal(chunks.cpu()[:, 0], torch.from_numpy(R.gather(x, L, m, f))), "case e: the gathered chunks differ from the oracle's"
    stub = Stub(L).to(device)
    y = stub(chunks)
    out, obuf = guarded(np.full(T, np.nan, np.float32), device, guard=SENTINEL)
    ramp = inf.chunk_ramp(f, "hann").to(device)
    assert np.array_equal(ramp.cpu().numpy(), R.ramp(f, "hann"))
    eng.chunk_overlap_add(y, torch.from_numpy(recs).to(device), out, m, f, ramp, T)
    check_against(reference_for(x, L, m, f, "hann", stub=stub), out, "case e, guarded arrays")
    assert bit_equal(fbuf, before) and bool((obuf[:1] == SENTINEL).all() and (obuf[1 + T:] == SENTINEL).all()), "case e: a guard was touched"
    # the same through enhance(), the mixture being the unaligned view
    res = inf.enhance(Stub(L).to(device), flat.view(1, 1, T), sample_length=L, margin=m, fade=f, engine=engine)
    assert bit_equal(res.reshape(-1), out) and bit_equal(fbuf, before)


def check_many(engine, device, window, identity=False):
    """Case f: enhance_many with max_batch = 3 against enhance of each recording alone (bit for bit) and against the oracle."""
    L, m, f, lengths = CASES["f"]
    inf = inference()
    xs = [recording(T, seed=1) for T in lengths]
    stub = Stub(L, identity=identity).to(device)
    recs = [torch.from_numpy(np.array(x)).to(device).view(1, 1, -1) if i % 2 == 0 else torch.from_numpy(np.array(x)).to(device) for i, x in enumerate(xs)]
    outs = inf.enhance_many(stub, recs, sample_length=L, max_batch=3, margin=m, fade=f, window=window, engine=engine)
    n = sum(R.count(T, L, m, f) for T in lengths)
    assert sum(s.shape[0] for s in stub.seen) == n and max(s.shape[0] for s in stub.seen) <= 3
    assert len(stub.seen) > len(lengths)                   # (more slabs than recordings: they straddle)
    assert bit_equal(torch.cat(stub.seen).cpu()[:, 0], torch.from_numpy(np.concatenate([R.gather(x, L, m, f) for x in xs])))
    assert len(outs) == len(xs)
    for x, rec, out in zip(xs, recs, outs):
        assert out.shape == rec.shape
        alone = enhance_one(engine, device, x, L, m, f, window, Stub(L, identity=identity).to(device))
        assert bit_equal(out.reshape(-1), alone.reshape(-1)), f"case f T {len(x)} {window}: enhance_many differs from enhance"
        check_against(reference_for(x, L, m, f, window, stub=stub), out, f"case f T {len(x)} {window}")
    # margin = fade = 0: the table-driven pass equals enhance's code path of before
    stub0 = Stub(L).to(device)
    outs0 = inf.enhance_many(stub0, recs, sample_length=L, max_batch=3, engine=engine)
    for x, out in zip(xs, outs0):
        alone = inf.enhance(Stub(L).to(device), torch.from_numpy(np.array(x)).to(device).view(1, 1, -1), sample_length=L, max_batch=3)
        assert bit_equal(out.reshape(-1), alone.reshape(-1)), f"case f T {len(x)}, margin = fade = 0"


def check_recorded(engine, device, inner, L, m, f, T, window="hann", label="real size", **kw):
    """Cases g / h: any model; the oracle is fed with the chunk outputs the device produced."""
    x = recording(T, seed=2)
    model = Recorder(inner)
    out = enhance_one(engine, device, x, L, m, f, window, model, **kw)
    given, said = torch.cat(model.seen).cpu()[:, 0], torch.cat(model.said).cpu()[:, 0]
    g = R.gather(x, L, m, f) if T <= 4096 else None
    if g is None:                                          # (the loop form of the oracle's gather is for the small cases)
        H, n = R.hop(L, m, f), R.count(T, L, m, f)
        idx = (np.arange(n) * H - m)[:, None] + np.arange(L)[None, :]
        g = np.where((idx >= 0) & (idx < T), x[np.clip(idx, 0, T - 1)], np.float32(0.0)).astype(np.float32)
    assert bit_equal(given, torch.from_numpy(g)), f"{label}: the gathered chunks differ from the oracle's"
    ref = reference_for(x, L, m, f, window, said=said.numpy())
    check_against(ref, out, label)
    return out, ref
