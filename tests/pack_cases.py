"""Inputs for the model-input packers, shared by tests/test_pack_cpu.py (kgpu_pack_host against tests/pack_ref.py) and tests/test_gpu_pack.py (the device
against both): ragged id arrays and the sweep of option combinations.  Plain Python over pack_ref's constants; imports without a device."""
import pack_ref as P


def ragged(rng, lengths_a, lengths_b=None):
    """Sequences of the given RAW lengths back to back in one id array behind 1 - 3 leading elements (the first sequence does not start at 0, and the
    offsets are odd and even as the lengths fall), the pairs' b sequences behind all the a's: off_b is the tail of one offsets array, the layout the
    Python layer produces.  -> ids, off_a, off_b (None for singles), spans_in, tix_in."""
    n = len(lengths_a)
    flat = [rng.randrange(1, 4)]
    for ln in list(lengths_a) + (list(lengths_b) if lengths_b is not None else []):
        flat.append(flat[-1] + ln)
    total = flat[-1] + rng.randrange(3)
    ids = [rng.choice((rng.randrange(-2**31, 2**31), rng.randrange(0, 32000))) for _ in range(total)]
    spans = [tuple(rng.randrange(2**32) for _ in range(4)) for _ in range(total)]
    tix = [rng.randrange(-1, 2**31) for _ in range(total)]
    return ids, flat[: n + 1], (flat[n:] if lengths_b is not None else None), spans, tix


def sweep_calls(max_length, rng, samples_per_call=None):
    """Every (singles | pairs) x strategy x windows of one max_length, each with the strides {0, 1, room - 1 (w - 1 beside an empty fixed side), room - 2
    (w - 1 beside a fixed side of one)} and every trim combination (from max_length 64: one, all four coming round), over samples whose TRIMMED lengths are drawn from
    {0, 1, room - 1, room, room + 1, room + step, 3 room}: all of them (singles) or all pairs of them (pairs), or samples_per_call seeded picks."""
    trim_cycle = 0
    for pair in (False, True):
        ns = 3 if pair else 2
        if max_length < ns + 1:
            continue
        room = max_length - ns
        for strategy in (P.LONGEST_FIRST, P.ONLY_FIRST, P.ONLY_SECOND):
            for windows in (False, True):
                if (strategy == P.ONLY_SECOND and not pair) or (strategy == P.LONGEST_FIRST and windows):
                    continue
                for stride in sorted({s for s in (0, 1, room - 1, room - 2) if 0 <= s < room}):
                  trim_cycle += 1
                  for tf, tb in ((0, 0), (0, 1), (1, 0), (1, 1)) if max_length <= 17 else ((trim_cycle & 1, (trim_cycle >> 1) & 1),):
                    step = room - stride
                    lens = sorted({v for v in (0, 1, room - 1, room, room + 1, room + step, 3 * room) if v >= 0})
                    combos = [(a, b) for a in lens for b in lens] if pair else [(a, None) for a in lens]
                    if samples_per_call and len(combos) > samples_per_call:
                        combos = rng.sample(combos, samples_per_call)
                    raw = lambda v: v + tf + tb   # noqa: E731
                    la = [raw(a) for a, _ in combos] + [0, 1, tf + tb]                      # (and sequences no longer than their trims)
                    lb = [raw(b) for _, b in combos] + [1, 0, tf + tb] if pair else None
                    yield dict(max_length=max_length, stride=stride, strategy=strategy, windows=windows, trim_front=tf, trim_back=tb, cls_id=-5, sep_id=2**31 - 1,
                               pad_id=-2**31), la, lb
