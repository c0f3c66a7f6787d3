"""What the GPU test modules of the analysis side (tests/test_gpu_pitch.py ... tests/test_gpu_auditory.py) share.  A plain module, imported the
way voice_stubs and the *_ref modules are: no fixture, hook or marker lives here, and it imports without a GPU.  A new analysis family starts
from it: its module keeps ``load``, the marshalling of ``raw``, ``check``, its tables of bad arguments and its tests.

  * ``Guarded``: the outputs of one raw call, each between two sentinel margins, and the rule every call is held to (``collect``);
  * ``frozen``: a reference computed once and never written again;
  * ``err_of``, ``engine_with``, ``one_engine``, ``engines_on_demand``: the engines; the last two are the bodies of module-scoped fixtures, which
    stay declared in each module (``yield from``).
tests/test_analysis_gpu_host.py drives ``Guarded`` and ``frozen`` on the CPU.
"""
import numpy as np
import torch

from emojivoice_amd._lib import Engine

DEV = "cuda:0"
M = 64                                   # sentinel margin, elements


def default_fill(dtype):
    return 777.0 if dtype.is_floating_point else {torch.int32: -777, torch.uint8: 77}[dtype]


class Guarded:
    """Output buffers for one call of the library: ``spec`` is {name: (shape, dtype)} in the call's order, ``fills`` {name: value} replaces the
    dtype's sentinel value for an output, ``null`` names the outputs passed as NULL."""

    def __init__(self, spec, null=(), fills=None, device=DEV):
        self.null, self.device, self.out = tuple(null), device, {}
        for name, (shape, dtype) in spec.items():
            shape, fill = tuple(int(s) for s in shape), (fills or {}).get(name, default_fill(dtype))
            n = int(np.prod(shape))
            self.out[name] = (torch.full((n + 2 * M,), fill, dtype=dtype, device=device), shape, n, fill)

    def ptr(self, name):
        """The address of the payload, or None where the output is passed as NULL."""
        whole, _, n, _ = self.out[name]
        return None if name in self.null else whole[M: M + n].data_ptr()

    def collect(self, rc):
        """After the call (synchronises the device first): every margin still holds its fill; an output passed as NULL, and every output of a
        failed call (``rc`` != 0), is untouched and comes back None; the others come back as host copies in their shapes -> {name: array}."""
        if self.device != "cpu":
            torch.cuda.synchronize()
        res = {}
        for name, (whole, shape, n, fill) in self.out.items():
            view = whole[M: M + n]
            assert bool((whole[:M] == fill).all()) and bool((whole[M + n:] == fill).all()), f"sentinel margin of d_{name}"
            if rc != 0 or name in self.null:
                assert bool((view == fill).all()), f"d_{name} was not asked for (or the call failed) and was written"
                res[name] = None
            else:
                res[name] = view.reshape(shape).cpu().numpy().copy()
        return res


def _freeze(r):
    if isinstance(r, np.ndarray):
        r.setflags(write=False)
    elif isinstance(r, (dict, tuple, list)):
        for v in (r.values() if isinstance(r, dict) else r):
            _freeze(v)


def frozen(cache, key, make):
    """``cache[key]``, made by ``make()`` on the first lookup; every ndarray in it (dicts, tuples and lists, nested) is set read-only."""
    if key not in cache:
        r = make()
        _freeze(r)
        cache[key] = r
    return cache[key]


def err_of(eng):
    return eng.lib.ev_last_error(eng.h).decode()


def engine_with(load=None, *args):
    """An Engine without weights, after ``load(engine, *args)`` returned 0 where a load is given."""
    e = Engine(0)                                                        # no weights loaded
    assert load is None or load(e, *args) == 0, err_of(e)
    return e


def one_engine(load=None, *args):
    """Fixture body: one engine (``engine_with``), closed at teardown."""
    e = engine_with(load, *args)
    yield e
    e.close()


def engines_on_demand(make):
    """Fixture body: get(key) -> ``make(key)``, made on the first request and closed at teardown."""
    made = {}

    def get(key):
        if key not in made:
            made[key] = make(key)
        return made[key]
    yield get
    for e in made.values():
        e.close()
