"""The step seed of the dropout masks, in device memory.

A model's `_Program` normally draws its mask seed on the host, once per forward.  A captured training step bakes that
scalar into its launches, so every replay would repeat the masks.  `attach(model)` puts a 4-word state
`{base, step, cur, 0}` on the model's device instead; `vc_seed_next` (one launch, first in every step) advances it,

    step += 1;  cur = splitmix64(base + step * 0x9E3779B97F4A7C15) >> 2        (64-bit wrapping; cur < 2^62)

and the `_ds` entry points read `cur` there, adding the site's offset `1000003 * k` as the host does.  `cur` is a pure
function of `(base, step)`: `step_seed` restates it, so step n of a run uses `step_seed(base, n)` whether it ran
eagerly or as a replay, and a run is reproduced from its base.
"""
from __future__ import annotations

import torch

GOLDEN = 0x9E3779B97F4A7C15
SITE_STRIDE = 1000003        # site k of a forward uses seed + SITE_STRIDE * k (program.py, hctnet.py)
_M64 = (1 << 64) - 1
_ATTR = "_vc_seed_state"


def splitmix64(z: int) -> int:
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def step_seed(base: int, step: int) -> int:
    """the seed of step `step` (1 for the first) of a run attached with `base`: what vc_seed_next leaves in `cur`"""
    return splitmix64((base & _M64) + (step & _M64) * GOLDEN) >> 2


def site_offset(k: int) -> int:
    return SITE_STRIDE * k


def host_seed() -> int:
    """one draw from torch's CPU generator with the rank mixed in: a forward's mask seed (program.seed_dropout) or an
    attached state's base.  The same `torch.manual_seed` reproduces a run; under data parallelism every rank seeds
    torch alike, so the replicas must differ here -- they must not apply the same keep masks to their shards"""
    from .parallel import rank
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return (seed + GOLDEN * rank()) % (1 << 62)


def _i64(v: int) -> int:
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


class SeedState:
    """{base, step, cur, 0} as four 64-bit words on `device`"""

    def __init__(self, base: int, device):
        self.base = int(base) & _M64
        self.buf = torch.tensor([_i64(self.base), 0, 0, 0], dtype=torch.int64, device=device)

    @property
    def device(self):
        return self.buf.device

    @property
    def state_ptr(self) -> int:
        return self.buf.data_ptr()

    @property
    def cur_ptr(self) -> int:
        return self.buf.data_ptr() + 16

    def advance(self, stream=None):
        """vc_seed_next on `stream` (a raw handle; default: torch's current stream of the state's device)"""
        from ._lib import lib
        if stream is None:
            stream = torch.cuda.current_stream(self.buf.device).cuda_stream
        lib().vc_seed_next(self.buf.data_ptr(), stream)

    def read(self):
        """(base, step, cur) as Python ints; synchronises"""
        b, s, c, _ = (int(v) & _M64 for v in self.buf.tolist())
        return b, s, c


def attach(model, base: int | None = None) -> SeedState:
    """Give `model` (on its ROCm device already) a device-resident step seed starting at step 0.  While one is
    attached and the model trains, its forwards draw nothing on the host and read the seed on the device; whoever
    steps the model advances it first (`TrainStepper` does, or `state(model).advance()`)."""
    flat = getattr(model, "_flat_store", None)
    if flat is None:
        raise TypeError("seeds.attach expects one of the package's flat-parameter models")
    if flat.device.type != "cuda":
        raise RuntimeError("seeds.attach: move the model to its ROCm (cuda) device first")
    st = SeedState(host_seed() if base is None else base, flat.device)
    object.__setattr__(model, _ATTR, st)
    return st


def detach(model) -> None:
    if getattr(model, _ATTR, None) is not None:
        object.__setattr__(model, _ATTR, None)


def state(model) -> SeedState | None:
    return getattr(model, _ATTR, None)


def state_for(model, device) -> SeedState | None:
    """the attached state for a forward on `device` (None: the host draws the seed, as without this module)"""
    st = getattr(model, _ATTR, None)
    if st is not None and st.buf.device != device:
        raise RuntimeError("the model's device seed is on another device: seeds.attach(model) again after moving it")
    return st


def has_dropout(model) -> bool:
    """does a training forward of `model` draw a mask (an nn.Dropout with p > 0, or the ViT models' p_drop / p_emb) or
    other noise from the step seed (`draws_noise`: MHST's head gates)"""
    if getattr(model, "draws_noise", False) or getattr(model, "p_drop", 0.0) > 0 or getattr(model, "p_emb", 0.0) > 0:
        return True
    return any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in model.modules())
