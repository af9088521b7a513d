"""-m "not gpu": the CALL PLAN of ``sliding_window_inference`` -- every library entry (tests/launch_trace.py: recorded, nothing launched), every predictor and
``process_fn`` invocation, every ``shard.agree_batch`` / ``shard.gather_round`` and the result's type, shape and dtype, in one list per case -- is pinned to text
fixtures (tests/golden/inferer_plans/<case>.txt).  A restructuring of the inferer that adds a launch, a copy through the library, a collective or a predictor call,
or that shows a predictor a batch twice, fails here.  The predictors are stubs that only record (real networks: tests/test_launch_plans.py); the tensors are CPU
tensors whose values are never read.  Two answers of the library that the plan depends on are given for real: ``mh_sw_mosaic_class_counts`` (host arithmetic that
sizes the mosaic) is executed, and ``mh_sw_blend_argmax_f32`` refuses an irregular window grid by the library's own rule (csrc/capi.hip: regular_axis), restated
below.  Not visible on CPU tensors: the free-memory agreement inside the window-major allocation (it is made for ROCm devices only).
``python tests/test_inferer_plans.py`` rewrites the fixtures (do that only for a change that is MEANT to move calls)."""
import contextlib
import os
import socket
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PLANS = os.path.join(HERE, "golden", "inferer_plans")
K = 3
VOL = (1, 1, 64, 48, 48)         # roi 32^3 at overlap 0.5: 3 x 2 x 2 = 12 windows
ROW_BYTES = 4 * K * 32 ** 3 * 4  # the logits of one row of windows along the first axis


def _regular_axis(s) -> bool:
    n = len(s)
    if s[0] != 0:
        return False
    if n <= 2:
        return True
    step = s[1]
    return step >= 1 and all(s[i] == i * step for i in range(1, n - 1)) and (n - 2) * step < s[-1] <= (n - 1) * step


@contextlib.contextmanager
def _recording():
    from launch_trace import launch_trace
    from monai_amd import _lib

    with launch_trace() as lines:
        lib = _lib.lib()
        record = lib.call

        def call(name, *args):
            record(name, *args)
            if name == "mh_sw_mosaic_class_counts":
                lib.check(lib._mh_sw_mosaic_class_counts(*args))
            if name == "mh_sw_blend_argmax_f32" and not all(_regular_axis(list(args[i])) for i in (12, 14, 16)):
                raise _lib.KernelRejected("monai_amd: sw_blend_argmax: irregular window starts (blend, then argmax) (code 2)")

        lib.call = call
        yield lines


def _coords(coords) -> str:
    return " ".join("[" + ",".join(f"{s.start}:{s.stop}" for s in c) + "]" for c in coords)


class Engine:
    """what the inferer asks of a fused network: ``out_channels``, ``forward_into`` (rows of the window-major buffer), ``forward_into_windows`` (the mosaic)"""

    out_channels = K

    def __init__(self, log):
        self.log = log

    def forward_into(self, x, out):
        r0 = out.storage_offset() // out.stride(0)
        self.log.append(f"forward_into {tuple(x.shape)} rows {r0}:{r0 + out.shape[0]} of {tuple(out.shape[1:])} stride {out.stride(0)}")

    def forward_into_windows(self, x, mosaic, w0):
        self.log.append(f"forward_into_windows {tuple(x.shape)} w0 {w0} mosaic k {mosaic.k} floats {mosaic.total}")

    def __call__(self, x, *args, **kwargs):
        self.log.append(f"engine call {tuple(x.shape)}")
        return torch.zeros((x.shape[0], K) + tuple(x.shape[2:]))


def _generic(log, form="tensor"):
    """a plain callable: one tensor, a tuple with a half-resolution second output, or a dict of two outputs"""
    def predictor(x, *args, **kwargs):
        coords = args[0] if args and isinstance(args[0], list) else None
        log.append(f"predictor {tuple(x.shape)} {x.dtype}" + (" coords " + _coords(coords) if coords is not None else "") + (f" kwargs {sorted(kwargs)}" if kwargs else ""))
        a = torch.cat([x, x], dim=1)
        if form == "tuple":
            return a, torch.nn.functional.avg_pool3d(a, 2)
        if form == "dict":
            return {"seg": a, "aux": x}
        return a

    return predictor


def _process_fn(log):
    def process_fn(segs, win_data, imp):
        log.append(f"process_fn {[tuple(s.shape) for s in segs]} windows {tuple(win_data.shape)} map {tuple(imp.shape)}")
        return segs, imp

    return process_fn


class Meta(torch.Tensor):
    """the two things the inferer asks of a MetaTensor: ``as_tensor`` and ``copy_meta_from``"""

    def __new__(cls, x):
        return x.as_subclass(cls)

    def as_tensor(self):
        return self.as_subclass(torch.Tensor)

    def copy_meta_from(self, src, copy_attr=False):
        self.tag = getattr(src, "tag", None)


@contextlib.contextmanager
def _env(**values):
    saved = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _one_rank_forced(log):
    import torch.distributed as dist

    from monai_amd import parallel

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    real = (parallel.WindowShard.agree_batch, parallel.WindowShard.gather_round)

    def agree_batch(self, nb, device):
        log.append(f"agree_batch {nb}")
        return real[0](self, nb, device)

    def gather_round(self, full, q, nb):
        log.append(f"gather_round q {q} nb {nb} buffer {tuple(full.shape)}")
        return real[1](self, full, q, nb)

    parallel.WindowShard.agree_batch, parallel.WindowShard.gather_round = agree_batch, gather_round
    try:
        with parallel.window_sharding(force=True):
            yield
    finally:
        parallel.WindowShard.agree_batch, parallel.WindowShard.gather_round = real
        dist.destroy_process_group()


def _describe(result) -> list:
    if isinstance(result, dict):
        parts = [(f"dict[{k!r}]", v) for k, v in result.items()]
    elif isinstance(result, (tuple, list)):
        parts = [(f"{type(result).__name__}[{i}]", v) for i, v in enumerate(result)]
    else:
        parts = [("result", result)]
    return [f"{name} {type(v).__name__} {tuple(v.shape)} {v.dtype}" + (f" tag {v.tag}" if hasattr(v, "tag") else "") for name, v in parts]


def _run(log, x, predictor, roi=(32, 32, 32), sw_batch_size=4, argmax=None, expect=None, **kw):
    """one call; `expect`: the exception type the case is about (recorded with its message; anything else propagates)"""
    from monai_amd.inferers import sliding_window_argmax, sliding_window_inference

    kw.setdefault("overlap", 0.5)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            if argmax is not None:
                out = sliding_window_argmax(x, roi, sw_batch_size, predictor, labels_dtype=argmax, **kw)
            else:
                out = sliding_window_inference(x, roi, sw_batch_size, predictor, **kw)
        log.extend(f"warning {w.category.__name__}: {w.message}" for w in caught)
        log.extend(_describe(out))
    except Exception as e:
        if expect is None or type(e).__name__ != expect:
            raise
        log.append(f"raises {type(e).__name__}: {e}")


def _errors(log):
    """the six argument errors in their order: each call also breaks every LATER rule, so the first one raised is the one pinned"""
    bad = torch.zeros(1, 1, 4, 4, 4, 4, requires_grad=True)      # four spatial dims, requires grad
    pred = _generic(log)
    for expect, kw in (("ValueError", dict(buffer_steps=1, buffer_dim=9, overlap=1.0, argmax=torch.uint8)),
                       ("NotImplementedError", dict(buffer_steps=1, buffer_dim=4, overlap=1.0, argmax=torch.uint8)),
                       ("NotImplementedError", dict(buffer_steps=1, buffer_dim=0, overlap=1.0, argmax=torch.uint8)),
                       ("ValueError", dict(overlap=1.0)),
                       ("NotImplementedError", dict()),
                       ("NotImplementedError", dict(x=torch.zeros(1, 1, 8, 8, 8, requires_grad=True)))):
        n0 = len(log)
        _run(log, kw.pop("x", bad), pred, roi=4, sw_batch_size=1, expect=expect, **kw)
        assert len(log) == n0 + 1, "an argument error must be raised before any call"


def _case(name: str, log: list) -> None:
    x = torch.zeros(VOL)
    eng = Engine(log)
    strict = _env(MONAI_AMD_STRICT_SW_BATCH=1)      # the engine is given sw_batch_size windows per launch: three rounds instead of one
    cap = _env(MONAI_AMD_MAX_LOGITS_BYTES=2.5 * ROW_BYTES)       # two rows of windows fit, the three of the volume do not
    if name == "fused_mosaic":
        with strict:
            _run(log, x, eng, mode="gaussian")
    elif name == "fused_auto_batch_b2":           # the engine's own launch size, two images
        _run(log, torch.zeros((2,) + VOL[1:]), eng, mode="gaussian")
    elif name == "fused_windows":
        with strict, _env(MONAI_AMD_LOGITS_LAYOUT="windows"):
            _run(log, x, eng, mode="gaussian")
    elif name == "engine_with_kwargs":            # a keyword of the predictor's own: the engine is called like any callable
        _run(log, x, eng, flag=True)
    elif name == "fused_argmax_u8":
        with strict:
            _run(log, x, eng, argmax=torch.uint8)
    elif name == "argmax_irregular":              # half-resolution starts 0 2 5 7: the library refuses, blend + channel argmax
        _run(log, torch.zeros(1, 1, 35, 20, 20), _generic(log, "tuple"), roi=(20, 20, 20), overlap=0.75, argmax=torch.float32)
    elif name == "fused_buffered":
        with strict:
            _run(log, x, eng, buffer_steps=2, buffer_dim=0)
    elif name == "generic_tuple":
        _run(log, x, _generic(log, "tuple"), mode="gaussian")
    elif name == "generic_dict":
        _run(log, x, _generic(log, "dict"), flag=True)            # + a keyword argument of the predictor's own
    elif name == "process_fn":
        _run(log, x, _generic(log, "tuple"), process_fn=_process_fn(log))
    elif name == "with_coord":
        _run(log, x, _generic(log), with_coord=True)
    elif name == "buffered_callbacks":
        _run(log, x, _generic(log), sw_batch_size=3, process_fn=_process_fn(log), with_coord=True, buffer_steps=2, buffer_dim=1)
    elif name == "buffered_dict":
        _run(log, x, _generic(log, "dict"), buffer_steps=1, buffer_dim=-1)
    elif name == "slabwise":
        with strict, cap:
            _run(log, x, eng, mode="gaussian")
            _run(log, x, _generic(log, "tuple"))
    elif name == "buffered_does_not_fit":
        with strict, cap:
            _run(log, x, eng, buffer_steps=2, buffer_dim=0)
    elif name == "buffered_does_not_fit_process_fn":
        with cap:
            n0 = len(log)
            _run(log, x, eng, process_fn=_process_fn(log), buffer_steps=2, buffer_dim=0, expect="_LogitsDoNotFit")
            assert len(log) == n0 + 1, "the fit decision must precede the first predictor call"
    elif name == "padded":
        with strict:
            _run(log, torch.zeros(1, 1, 64, 48, 20), eng)
        _run(log, torch.zeros(1, 1, 64, 48, 20), _generic(log, "tuple"), padding_mode="replicate")
    elif name == "two_d":
        _run(log, torch.zeros(1, 1, 48, 48), _generic(log), roi=(32, 32), mode="gaussian")
    elif name == "float16":
        with strict:
            _run(log, x.half(), eng)
        _run(log, x.bfloat16(), _generic(log, "dict"))
    elif name == "meta_tensor":
        m = Meta(x)
        m.tag = "kept"
        with strict:
            _run(log, m, eng)
            with cap:
                _run(log, m, eng)
        _run(log, m.half(), _generic(log, "tuple"))
    elif name == "sharded_one_rank":
        with _one_rank_forced(log):
            _run(log, x, eng, mode="gaussian")
            _run(log, x, _generic(log, "tuple"))
    elif name == "argument_errors":
        _errors(log)
    else:
        raise KeyError(name)


NAMES = ("fused_mosaic", "fused_auto_batch_b2", "fused_windows", "engine_with_kwargs", "fused_argmax_u8", "argmax_irregular", "fused_buffered", "generic_tuple", "generic_dict",
         "process_fn", "with_coord", "buffered_callbacks", "buffered_dict", "slabwise", "buffered_does_not_fit", "buffered_does_not_fit_process_fn", "padded",
         "two_d", "float16", "meta_tensor", "sharded_one_rank", "argument_errors")


def _trace(name: str) -> list:
    with _recording() as lines, _env(MONAI_AMD_NO_FALLTHROUGH=1):
        _case(name, lines)
    return list(lines)


@pytest.mark.parametrize("name", NAMES)
def test_inferer_plan(name):
    lines = _trace(name)
    with open(os.path.join(PLANS, name + ".txt")) as f:
        want = f.read().splitlines()
    for i, (a, b) in enumerate(zip(lines, want)):
        assert a == b, f"call {i}: {a!r} != {b!r}"
    assert len(lines) == len(want), (len(lines), len(want))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.makedirs(PLANS, exist_ok=True)
    for nm in NAMES:
        with open(os.path.join(PLANS, nm + ".txt"), "w") as f:
            f.write("\n".join(_trace(nm)) + "\n")
