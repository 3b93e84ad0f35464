"""The cases of tests/test_gpu_window_limits.py (tests/window_cases.py) without a device: every scenario's sentences are on the intended side of their limit by the oracle's node
counts and the key lists alone (the scenarios_* functions assert that while they build the cases), the arena batches have the lengths the test
counts on, and every limit from 1 to 8 has a held and a handed sentence."""
import window_cases as L


def test_every_case_is_on_its_side_of_its_limit():
    whys = {}
    for make in L.ALL_SCENARIOS:
        for sc in make():
            whys.setdefault(int(make.__name__[-1]), set()).update((sc.why, sc.team_why))
    assert whys == {k: {0, k} if k != 4 else {0, 4, 7} for k in (1, 2, 3, 4, 6, 7, 8)}, whys   # (5, a far chunk the arena cannot give, is the arena test's)


def test_arena_batches_outgrow_a_small_arena():
    from kanpyo_amd import Dict
    from oracle import oracle

    oracle.build()
    parts, plain, digits = L.arena_batches()
    orc = oracle.OracleTokenizer.from_dict(Dict.from_parts(**parts))
    for batch in (plain, digits):
        # one node chunk of 96 KB and a slab of 14 bytes per input byte (+ 50 %) per sentence, a sentence per workgroup: several times 1 MiB
        assert len(batch) * (96 << 10) + sum(len(s.encode()) * 21 for s in batch) > 4 << 20
        for s in batch[:4]:
            assert len(orc.tokenize(s)[0]) > 0
    assert all("1" * 200 in s for s in digits)   # runs longer than a window: far entries, a far chunk of 64 KB
