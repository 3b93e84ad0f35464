"""The waiting half of the device-resident calls, over fakes (no device, no library): what each of DeviceContext's sync methods returns and
raises for each answer of its entry point, and the one loop (_calls.device_call) that repeats a stage whose capacity was too small."""
import ctypes as C

import pytest

from kanpyo_amd import _calls, _lib
from kanpyo_amd.device import DeviceContext

CAPACITY = _lib.KGPU_ERR_CAPACITY
HANDLE = C.c_void_p(0x5150)


class FakeSyncs:
    """Stands where _lib.lib() stands: every kgpu_ctx_sync* entry answers .rc and writes .values through the references it was given."""

    ENTRIES = {"kgpu_ctx_sync": 1, "kgpu_ctx_sync_lines": 1, "kgpu_ctx_sync_count": 1, "kgpu_ctx_sync_normalize": 1, "kgpu_ctx_sync_normalize_aligned": 2,
               "kgpu_ctx_sync_split": 2}

    def __init__(self):
        self.rc, self.values, self.calls = 0, (11, 7), []

    def kgpu_last_error(self):
        return b"said the fake"

    def __getattr__(self, name):
        if name not in self.ENTRIES:
            raise AttributeError(name)

        def entry(h, *refs):
            assert h is HANDLE and len(refs) == self.ENTRIES[name]
            self.calls.append(name)
            for ref, v in zip(refs, self.values):
                ref._obj.value = v
            return self.rc

        return entry


@pytest.fixture
def ctx(monkeypatch):
    lib = FakeSyncs()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    c = DeviceContext.__new__(DeviceContext)
    c._h, c.lib = HANDLE, lib
    yield c
    c._h = None   # (nothing to destroy)


# method -> (entry point, what it returns when the entry wrote 11 and 7 and answered KGPU_OK)
SYNC = {"sync": ("kgpu_ctx_sync", 11), "sync_lines": ("kgpu_ctx_sync_lines", 11), "sync_count": ("kgpu_ctx_sync_count", 11),
        "sync_normalize": ("kgpu_ctx_sync_normalize", 11), "sync_normalize_aligned": ("kgpu_ctx_sync_normalize_aligned", (11, 7)),
        "sync_split": ("kgpu_ctx_sync_split", (11, 7))}
# method -> (entry point, what it returns for KGPU_OK, what it returns for KGPU_ERR_CAPACITY)
TRY_SYNC = {"try_sync": ("kgpu_ctx_sync", (True, 11), (False, 11)), "try_sync_lines": ("kgpu_ctx_sync_lines", (True, 11), (False, 11)),
            "try_sync_normalize": ("kgpu_ctx_sync_normalize", (True, 11), (False, 11)),
            "try_sync_normalize_aligned": ("kgpu_ctx_sync_normalize_aligned", (True, 11, 7), (False, 11, 7))}
OTHER_CODES = (_lib.KGPU_ERR_INVALID_ARG, _lib.KGPU_ERR_HIP, _lib.KGPU_ERR_INTERNAL)


@pytest.mark.parametrize("name", list(SYNC))
def test_sync_returns_the_sizes_and_raises_on_every_failure(ctx, name):
    entry, result = SYNC[name]
    got = getattr(ctx, name)()
    assert got == result and type(got) is type(result) and ctx.lib.calls == [entry]
    for code in (CAPACITY,) + OTHER_CODES:
        ctx.lib.rc = code
        with pytest.raises(_lib.KgpuError) as err:
            getattr(ctx, name)()
        assert err.value.code == code and "said the fake" in str(err.value)
    assert ctx.lib.calls == [entry] * 5   # (one call of the entry each, and of no other)


@pytest.mark.parametrize("name", list(TRY_SYNC))
def test_try_sync_returns_a_capacity_answer_and_raises_on_any_other(ctx, name):
    entry, fits, short = TRY_SYNC[name]
    assert getattr(ctx, name)() == fits
    ctx.lib.rc = CAPACITY
    assert getattr(ctx, name)() == short
    for code in OTHER_CODES:
        ctx.lib.rc = code
        with pytest.raises(_lib.KgpuError) as err:
            getattr(ctx, name)()
        assert err.value.code == code
    assert ctx.lib.calls == [entry] * 5


# ---- the loop over the attempts of one stage ----------------------------------------------------------------------------------------------------
def scripted(script):
    """An attempt that answers script[k] = (rc, reported) on its k-th call -> (the callable, the capacities it was called with)."""
    calls = []

    def attempt(*caps):
        rc, reported = script[len(calls)]
        calls.append(caps)
        return rc, reported, f"buffers of attempt {len(calls)}"

    return attempt, calls


def test_a_stage_that_fits_is_attempted_once_with_the_given_capacities():
    attempt, calls = scripted([(0, (9,))])
    assert _calls.device_call(attempt, (10,), slack=64) == ((9,), "buffers of attempt 1") and calls == [(10,)]
    attempt, calls = scripted([(0, [300, 2])])   # (a success is not repeated, whatever it reports)
    assert _calls.device_call(attempt, (10, 5)) == ((300, 2), "buffers of attempt 1") and calls == [(10, 5)]


@pytest.mark.parametrize("slack", [0, 64])
def test_a_capacity_too_small_is_one_more_attempt_with_the_reported_size(ctx, slack):
    attempt, calls = scripted([(CAPACITY, (25,)), (0, (25,))])
    assert _calls.device_call(attempt, (10,), slack=slack) == ((25,), "buffers of attempt 2") and calls == [(10,), (25 + slack,)]
    # two capacities: the one that fitted is kept (max(cap, reported + slack) is itself, or the reported size)
    for reported, second in (((25, 3), (25 + slack, max(5, 3 + slack))), ((7, 9), (max(10, 7 + slack), 9 + slack)), ((11, 6), (11 + slack, 6 + slack))):
        attempt, calls = scripted([(CAPACITY, reported), (0, reported)])
        assert _calls.device_call(attempt, (10, 5), slack=slack) == (reported, "buffers of attempt 2") and calls == [(10, 5), second]


def test_a_fixed_stage_is_attempted_once_and_its_capacity_answer_raises(ctx):
    attempt, calls = scripted([(CAPACITY, (25,)), (0, (25,))])
    with pytest.raises(_lib.KgpuError) as err:
        _calls.device_call(attempt, (10,), fixed=True)
    assert err.value.code == CAPACITY and calls == [(10,)]
    attempt, calls = scripted([(0, (25,))])
    assert _calls.device_call(attempt, (10,), fixed=True) == ((25,), "buffers of attempt 1")


def test_a_capacity_answer_with_every_size_within_capacity_raises(ctx):
    for reported in ((0, 0), (10, 5), (9, 4)):
        attempt, calls = scripted([(CAPACITY, reported)] * 3)
        with pytest.raises(_lib.KgpuError) as err:
            _calls.device_call(attempt, (10, 5), slack=64)
        assert err.value.code == CAPACITY and "said the fake" in str(err.value) and calls == [(10, 5)]


def test_another_error_raises_after_one_attempt(ctx):
    for code in OTHER_CODES:
        attempt, calls = scripted([(code, (99,))] * 2)
        with pytest.raises(_lib.KgpuError) as err:
            _calls.device_call(attempt, (10,))
        assert err.value.code == code and calls == [(10,)]
