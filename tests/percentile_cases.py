"""Shared cases of the percentile intensity transforms (ScaleIntensityRangePercentiles, ClipIntensityPercentiles) and of the order-statistic kernel
under them (monai_amd/csrc/kernels/select.h); tests/test_percentiles_emu.py runs them on the SIMT emulator, tests/test_percentiles_gpu.py on the MI355X.

Order statistics are compared with np.sort, independently of the reference.  The transforms are compared with the reference's own classes through
tests/golden/percentiles.npz (tests/golden/make_golden_percentiles.py); the inputs are regenerated here from seeds.

Which interpolation rule held in the torch.quantile regime (<= 1,000,000 elements per percentile call): the reference's CPU kernel evaluates at::lerp
with ONE fused multiply-add (w < 0.5 ? fma(w, b - a, a) : fma(w - 1, b - a, b)), not with a separately rounded product -- measured while making the
golden: over 2100 random cases the fused form reproduces torch.quantile bit for bit, the unfused form differs in 4.  The kernel uses the fused form,
so the percentile values are BIT-IDENTICAL to the reference's in both regimes (the numpy regime by construction: separately rounded ufuncs), the
issue's fp64-truth fallback rule is not needed, and every output is therefore required to be bit-identical to the golden as well."""
import inspect
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "percentiles.npz")
SHARE = 16384          # values per workgroup of the counting passes (select_parts, capi.hip): n <= SHARE is one workgroup
LENGTHS = (1, 2, 63, 64, 65, SHARE - 1, SHARE, SHARE + 1, 70001)
KINDS = ("normal", "ct256", "equal", "lowbits", "signexp", "mixed")
STRIDE = 997


# ------------------------------------------------------------------------------------------------------------------ order statistics
def run_data(kind: str, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return (rng.standard_normal(n) * 100).astype(np.float32)
    if kind == "ct256":                  # 256 levels: heavy ties, every rank is decided in the last pass
        return np.round(np.clip(rng.standard_normal(n) * 60 + 100, 0, 255)).astype(np.float32)
    if kind == "equal":
        return np.full(n, 3.5, np.float32)
    if kind == "lowbits":                # differ in the lowest mantissa bits only
        return (np.float32(1.0).view(np.uint32) + rng.integers(0, 8, n).astype(np.uint32)).view(np.float32)
    if kind == "signexp":                # differ in sign / exponent only
        return (np.ldexp(1.0, rng.integers(-20, 21, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    if kind == "mixed":                  # negatives, denormals, +-0, +-inf
        pool = np.array([-np.inf, np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -3.0, 2.5, -1e30, 1e30, 7.0], np.float32)
        x = pool[rng.integers(0, pool.size, n)]
        m = rng.random(n) < 0.5
        x[m] = (rng.standard_normal(int(m.sum())) * 1e-3).astype(np.float32)
        return x
    raise KeyError(kind)


def rank_sets(sorted0: np.ndarray):
    """lists of at most 4 ranks: the ends, adjacent pairs, and a pair whose two values fall in different first-pass bins of run 0 (where there is one)"""
    n = sorted0.size
    sets = [[0, n - 1]]
    if n >= 2:
        mid = (n - 1) // 2
        sets.append(sorted({0, 1, n - 2, n - 1}) if n < 4 else [mid, mid + 1, n - 2, n - 1])
        sets.append([min(n - 2, int(0.005 * (n - 1))), min(n - 2, int(0.005 * (n - 1))) + 1, int(0.995 * (n - 1)), min(n - 1, int(0.995 * (n - 1)) + 1)])
        s = sorted0.copy()
        s[s == 0] = 0.0
        u = s.view(np.uint32)
        key = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32) >> 21
        cut = np.nonzero(key[1:] != key[:-1])[0]
        if cut.size:
            k = int(cut[cut.size // 2])
            sets.append([k, k + 1])
    return sets


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    """equal by value, +-0 alike, NaN where NaN"""
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def case_order_statistics(dev, n: int, runs: int, first_kind: int, nan_run=None) -> int:
    from monai_amd import ops

    kinds = [KINDS[(first_kind + c) % len(KINDS)] for c in range(runs)]
    data = np.stack([run_data(k, n, 100 * first_kind + c) for c, k in enumerate(kinds)])
    if nan_run is not None:
        data[nan_run, (7 * n) // 11] = np.nan
    ref = np.sort(data, axis=1)
    x = torch.from_numpy(data).to(dev)
    checked = 0
    for ranks in rank_sets(np.sort(run_data(kinds[0], n, 100 * first_kind))):
        a = ops.order_statistics(x, runs, n, ranks).cpu().numpy()
        b = ops.order_statistics(x, runs, n, ranks).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("not the same bits twice", n, kinds, ranks)
        want = ref[:, ranks]
        if nan_run is not None:
            want[nan_run] = np.nan
        assert _same(a, want), (n, kinds, ranks, a, want)
        zero = a == 0
        assert not np.signbit(a[zero]).any(), "a selected zero is +0.0"
        checked += a.size
    assert torch.equal(x.cpu(), torch.from_numpy(data)) or nan_run is not None
    return checked


def case_order_statistics_errors(dev) -> None:
    import pytest
    from monai_amd import ops

    x = torch.arange(12, dtype=torch.float32).to(dev)
    for ranks in ([12], [-1], [0, 1, 2, 3, 4], []):
        with pytest.raises(RuntimeError):
            ops.order_statistics(x, 1, 12, ranks)
    with pytest.raises(RuntimeError):
        ops.order_statistics(x, 5, 2, [0])                 # 5 * 2 != 12
    with pytest.raises(ValueError, match=r"q values must be in \[0, 100\]"):
        ops.percentiles(x, 1, 12, [101.0])
    assert ops.order_statistics(x, 3, 4, [3]).cpu().flatten().tolist() == [3.0, 7.0, 11.0]


# ------------------------------------------------------------------------------------------------------------------ transforms vs the reference
DOC_IMAGE = [[[1, 2, 3, 4, 5]] * 6]

INPUT_SPECS = {             # name -> (shape, seed); float32 N(100, 300) quantised to 1/8 (ties, like stored intensities), regenerated wherever needed
    "small": ((2, 5, 7, 9), 11),
    "n999983": ((1, 999983), 12),
    "n1000000": ((1, 100, 100, 100), 13),
    "n1000001": ((1, 1000001), 14),
    "n1010000": ((1, 101, 100, 100), 15),
    "cw3": ((3, 70, 70, 70), 16),      # 343,000 per channel (torch.quantile's rule per channel), 1,029,000 as a whole (np.percentile's)
}
_inputs_cache: dict = {}


def inputs(name: str) -> np.ndarray:
    if name not in _inputs_cache:
        if name == "doc":
            a = np.asarray(DOC_IMAGE, np.float32)
        elif name == "const":
            a = np.full((2, 5, 6), 3.25, np.float32)
        else:
            shape, seed = INPUT_SPECS[name]
            a = (np.round(np.random.default_rng(seed).standard_normal(shape) * 300 * 8) / 8 + 100).astype(np.float32)
        a.setflags(write=False)
        _inputs_cache[name] = a
    return _inputs_cache[name]


def golden_cases():
    cases = []

    def add(inp, cls, form, **kw):
        cid = f"{inp}|{cls}{form}|" + ",".join(f"{k}={v}" for k, v in kw.items())
        cases.append({"id": cid, "inp": inp, "cls": cls, "form": form, "kw": kw})

    S, Cl = "ScaleIntensityRangePercentiles", "ClipIntensityPercentiles"
    # the reference's docstring examples, verbatim
    add("doc", S, "", lower=10, upper=90, b_min=0, b_max=200, clip=False, relative=False)
    add("doc", S, "", lower=10, upper=90, b_min=0, b_max=200, clip=False, relative=True)
    add("doc", Cl, "", lower=30, upper=70)
    pairs = ((0, 100), (0.5, 99.5), (10, 90), (30, 70), (40, 40))
    for inp in ("small", "const"):
        for lo, hi in pairs:
            for cw in (False, True):
                for form in ("", "d"):
                    for rel in (False, True):
                        for clip in (False, True):
                            if form == "d" and (rel != clip):       # the dictionary form: half of the grid
                                continue
                            add(inp, S, form, lower=lo, upper=hi, b_min=-1.5, b_max=2.0, clip=clip, relative=rel, channel_wise=cw)
                    add(inp, S, form, lower=lo, upper=hi, b_min=None, b_max=None, channel_wise=cw)
                    add(inp, S, form, lower=lo, upper=hi, b_min=0.25, b_max=None, clip=True, channel_wise=cw)
                    add(inp, S, form, lower=lo, upper=hi, b_min=None, b_max=1.0, clip=True, channel_wise=cw)
                    add(inp, Cl, form, lower=lo, upper=hi, channel_wise=cw)
                add(inp, Cl, "", lower=lo, upper=hi, channel_wise=cw, return_clipping_values=True)
        for cw in (False, True):
            add(inp, Cl, "", lower=None, upper=75, channel_wise=cw, return_clipping_values=True)
            add(inp, Cl, "d", lower=20, upper=None, channel_wise=cw)
    # both sides of the regime boundary of percentile(): 1,000,000 elements per call
    for inp in ("n999983", "n1000000", "n1000001", "n1010000", "cw3"):
        for cw in ((False, True) if inp == "cw3" else (False,)):
            add(inp, S, "", lower=0.5, upper=99.5, b_min=0, b_max=1, clip=True, channel_wise=cw)
            add(inp, S, "d", lower=10, upper=90, b_min=None, b_max=None, channel_wise=cw)
            add(inp, Cl, "", lower=0.5, upper=99.5, channel_wise=cw, return_clipping_values=True)
    return cases


def is_large(inp: str) -> bool:
    return inputs(inp).size > 100000


def run_case(mod, case, dev):
    """(output tensor, meta or None) of the case's transform taken from `mod` (the reference's monai.transforms, or monai_amd.transforms)"""
    x = torch.from_numpy(inputs(case["inp"]).copy()).to(dev)
    before = x.clone()
    if case["form"] == "d":
        out = getattr(mod, case["cls"] + "d")(keys="img", **case["kw"])({"img": x, "other": 1})
        assert out["other"] == 1
        out = out["img"]
    else:
        out = getattr(mod, case["cls"])(**case["kw"])(x)
    assert torch.equal(x, before), "the input was modified"
    return out, (dict(out.meta) if hasattr(out, "meta") else None)


def pct_args(case):
    kw = case["kw"]
    lo, hi = kw["lower"], kw["upper"]
    return (0 if lo is None else lo), (100 if hi is None else hi)


_golden_cache: dict = {}


def golden():
    if not _golden_cache:
        with np.load(GOLDEN) as z:
            _golden_cache.update({k: z[k] for k in z.files})
    return _golden_cache


def case_transforms_vs_golden(dev, which) -> int:
    """every golden case whose input is in `which`: the percentile values (a_min / a_max, through ops.percentiles) and the outputs bit-identical to the
    reference's; large inputs are compared on every 997th value and the fp64 sum"""
    import monai_amd.transforms as ours
    from monai_amd import ops

    g = golden()
    assert json.loads(str(g["manifest"])) == [c["id"] for c in golden_cases()], "tests/golden/percentiles.npz is stale: run make_golden_percentiles.py"
    n_checked = 0
    for case in golden_cases():
        if case["inp"] not in which:
            continue
        cid = case["id"]
        x = torch.from_numpy(inputs(case["inp"]).copy()).to(dev)
        c = x.shape[0] if case["kw"].get("channel_wise") else 1
        table = ops.percentiles(x, c, x.numel() // c, pct_args(case)).cpu().numpy()
        assert np.array_equal(table.view(np.uint32), g[cid + "|pct"]), (cid, table, g[cid + "|pct"].view(np.float32))
        out, meta = run_case(ours, case, dev)
        assert out.dtype == torch.float32 and tuple(out.shape) == inputs(case["inp"]).shape, cid
        o = torch.as_tensor(out).cpu().numpy().reshape(-1)
        if is_large(case["inp"]):
            assert np.array_equal(o[::STRIDE].view(np.uint32), g[cid + "|samp"]), cid
            assert float(o.astype(np.float64).sum()) == float(g[cid + "|sum"]), cid
        else:
            assert np.array_equal(o.view(np.uint32), g[cid + "|out"].reshape(-1)), (cid, o[:8], g[cid + "|out"].reshape(-1)[:8].view(np.float32))
        if case["kw"].get("return_clipping_values"):
            cv = meta["clipping_values"]
            assert isinstance(cv, list) and all(isinstance(t, tuple) and len(t) == 2 for t in cv), cv
            assert np.array_equal(np.asarray(cv, np.float64), g[cid + "|clipvals"]), (cid, cv, g[cid + "|clipvals"])
        n_checked += 1
    assert n_checked
    return n_checked


def case_doc_examples(dev) -> None:
    """the two docstrings of the reference, by their printed values"""
    import monai_amd.transforms as ours

    img = torch.tensor(DOC_IMAGE, dtype=torch.float32).to(dev)
    row = lambda *v: torch.tensor([[list(v)] * 6], dtype=torch.float32)        # noqa: E731
    assert torch.equal(ours.ScaleIntensityRangePercentiles(10, 90, 0, 200, False, False)(img).cpu(), row(0, 50, 100, 150, 200))
    assert torch.equal(ours.ScaleIntensityRangePercentiles(10, 90, 0, 200, False, True)(img).cpu(), row(20, 60, 100, 140, 180))
    assert torch.equal(ours.ClipIntensityPercentiles(30, 70)(img).cpu(), row(2, 2, 3, 4, 4))


def case_nan_and_determinism(dev) -> None:
    """a NaN in one channel: that channel's percentiles (and so its output) are NaN, the others are untouched; two calls give the same bits"""
    import monai_amd.transforms as ours

    a = inputs("small").copy()
    a[1, 3, 4, 5] = np.nan
    x = torch.from_numpy(a).to(dev)
    t = ours.ScaleIntensityRangePercentiles(5, 95, 0, 1, clip=True, channel_wise=True)
    o1, o2 = t(x).cpu().numpy(), t(x).cpu().numpy()
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32))
    assert np.isnan(o1[1]).all() and not np.isnan(o1[0]).any()
    clean = t(torch.from_numpy(inputs("small").copy()).to(dev)).cpu().numpy()
    assert np.array_equal(o1[0].view(np.uint32), clean[0].view(np.uint32))
    c = ours.ClipIntensityPercentiles(5, 95, channel_wise=True)(x).cpu().numpy()
    assert np.isnan(c[1]).all() and np.array_equal(c[0].view(np.uint32), ours.ClipIntensityPercentiles(5, 95)(x[:1]).cpu().numpy()[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ API
SIGNATURES = {      # parameter names and defaults of the reference (monai/transforms/intensity/array.py:1064-1072, 1364-1374; dictionary.py:902-911, 1055-1067)
    "ScaleIntensityRangePercentiles": "(lower, upper, b_min, b_max, clip=False, relative=False, channel_wise=False, dtype=float32)",
    "ClipIntensityPercentiles": "(lower, upper, sharpness_factor=None, channel_wise=False, return_clipping_values=False, dtype=float32)",
    "ScaleIntensityRangePercentilesd": "(keys, lower, upper, b_min, b_max, clip=False, relative=False, channel_wise=False, dtype=float32, allow_missing_keys=False)",
    "ClipIntensityPercentilesd": "(keys, lower, upper, sharpness_factor=None, channel_wise=False, dtype=float32, allow_missing_keys=False)",
}


def signature_text(cls) -> str:
    ps = list(inspect.signature(cls.__init__).parameters.values())[1:]
    fmt = lambda d: "float32" if d is np.float32 else repr(d)        # noqa: E731
    return "(" + ", ".join(p.name if p.default is p.empty else f"{p.name}={fmt(p.default)}" for p in ps) + ")"


def case_api(dev) -> None:
    import pytest
    import monai_amd.transforms as ours
    from monai_amd.data.meta_tensor import MetaTensor

    for name, text in SIGNATURES.items():
        assert signature_text(getattr(ours, name)) == text, name
    for base in ("ScaleIntensityRangePercentiles", "ClipIntensityPercentiles"):
        assert getattr(ours, base + "D") is getattr(ours, base + "Dict") is getattr(ours, base + "d")
    S, Cl = ours.ScaleIntensityRangePercentiles, ours.ClipIntensityPercentiles
    for args in ((-1, 90, 0, 1), (101, 90, 0, 1), (10, -0.5, 0, 1), (10, 100.5, 0, 1)):
        with pytest.raises(ValueError, match=r"^Percentiles must be in the range \[0, 100\]$"):
            S(*args)
    for args in ((-1, 90), (10, 101), (None, 100.1), (-0.1, None)):
        with pytest.raises(ValueError, match=r"^Percentiles must be in the range \[0, 100\]$"):
            Cl(*args)
    with pytest.raises(ValueError, match="^upper must be greater than or equal to lower$"):
        Cl(60, 40)
    with pytest.raises(ValueError, match="^lower or upper percentiles must be provided$"):
        Cl(None, None)
    for sf in (0, -2.0):
        with pytest.raises(ValueError, match="^sharpness_factor must be greater than 0$"):
            Cl(10, 90, sharpness_factor=sf)
    with pytest.raises(NotImplementedError, match="soft clip"):
        Cl(10, 90, sharpness_factor=10.0)
    x = torch.from_numpy(inputs("small").copy()).to(dev)
    for b in ((None, 1.0), (0.0, None), (None, None)):
        with pytest.raises(ValueError, match=r"^If it is relative, b_min and b_max should not be None\.$"):
            S(10, 90, b[0], b[1], relative=True)(x)
    for bad in (x.to(torch.int16), x.to(torch.float64), x.to(torch.float16)):
        with pytest.raises(NotImplementedError, match="not on the HIP path"):
            S(10, 90, 0, 1)(bad)
        with pytest.raises(NotImplementedError, match="not on the HIP path"):
            Cl(10, 90)(bad)
    # MetaTensor in, MetaTensor out, meta and applied operations kept; the input is not modified; a plain tensor stays plain
    m = MetaTensor(x.clone(), meta={"affine": torch.eye(4), "name": "case"}, applied_operations=[{"class": "Earlier"}])
    for t in (S(10, 90, 0, 1, clip=True, channel_wise=True), Cl(10, 90), Cl(10, 90, return_clipping_values=True)):
        out = t(m)
        assert isinstance(out, MetaTensor) and out.meta["name"] == "case" and torch.equal(torch.as_tensor(out.meta["affine"]), torch.eye(4))
        assert out.applied_operations == [{"class": "Earlier"}]
        assert torch.equal(m.as_tensor(), x) and "clipping_values" not in m.meta
        plain = t(x)
        assert torch.equal(torch.as_tensor(plain).cpu(), out.as_tensor().cpu())
        if not getattr(t, "return_clipping_values", False):
            assert type(plain) is torch.Tensor
    assert S(10, 90, 0, 1, dtype=np.float64)(x).dtype == torch.float64 and S(10, 90, 0, 1, dtype=None)(x).dtype == torch.float32
    # dictionary forms: missing keys
    for D, kw in ((ours.ScaleIntensityRangePercentilesd, dict(lower=10, upper=90, b_min=0, b_max=1)), (ours.ClipIntensityPercentilesd, dict(lower=10, upper=90))):
        with pytest.raises(KeyError, match="was missing in the data and allow_missing_keys==False"):
            D(keys=("img", "absent"), **kw)({"img": x})
        out = D(keys=("img", "absent"), allow_missing_keys=True, **kw)({"img": x, "n": 3})
        assert set(out) == {"img", "n"} and out["n"] == 3 and not torch.equal(out["img"], x)
        assert isinstance(D(keys="img", **kw).scaler, (S, Cl))
