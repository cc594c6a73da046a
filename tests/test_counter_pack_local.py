"""The claim lc_counter_check_history's kernels rest on, proved on the CPU:
lc_counter_pack's serial fold equals the LOCAL rules of
csrc/counter_pack_plan.hpp (tests/counter_pack_helpers.py restates them) --
the keys, every key's error text, and the batch's arrays, for equality."""
import counter_pack_helpers as PH


def agree(rows, **kw):
    h = PH.hist(rows, **kw)
    want, _ = PH.host_pack(h)
    PH.same_batch(PH.local_pack(h), want)
    return want


def test_every_history_of_up_to_two_rows_and_a_deterministic_sample_up_to_six():
    """2 processes x {add, read} x 4 types x values {nil, -1, 1}: all 2,353 histories of at
    most 2 rows; of the 48^n of n = 3 .. 6 rows, 1,500 each, at a fixed stride coprime to 48."""
    A = len(PH.SMALL_ALPHABET)
    seen = set()
    for n in range(3):
        for i in range(A ** n):
            seen.update(e for e in agree(PH.small_history(n, i), keyed=False)["error"] if e)
    for n in range(3, 7):
        for j in range(1500):
            seen.update(e for e in agree(PH.small_history(n, (j * 1000003 + 17) % A ** n), keyed=False)["error"] if e)
    assert seen == set(PH.MESSAGES) - {PH.SUM}   # (values up to 1 cannot pass INT64_MAX)


def test_some_thousands_of_random_small_histories():
    rng = PH.rng_of(20240)
    offences = 0
    seen = set()
    for i in range(4000):
        rows = PH.random_rows(rng, rng.randrange(1, 65), rng.randrange(0, 4), rng.randrange(1, 5),
                              p_wild=rng.choice((0.0, 0.0, 0.03, 0.1)))
        want = agree(rows, keyed=rng.random() < 0.8, with_process=rng.random() < 0.9)
        offences += any(want["error"])
        seen.update(e for e in want["error"] if e)
    assert 800 < offences < 3200 and seen == set(PH.MESSAGES)


def test_the_lowest_row_decides_and_rule_one_goes_before_rule_three():
    I, O, F, A, R = PH.INVOKE, PH.OK, PH.FAIL, PH.ADD, PH.READ
    two = [(O, A, 0, None, 1), (I, R, 1, None, None), (I, R, 1, None, None)]
    assert agree(two, keyed=False)["error"] == [PH.NO_OPEN]
    assert agree(two[1:] + two[:1], keyed=False)["error"] == [PH.SECOND_INVOKE]
    # a negative add at row 0 (rule 3), an orphan completion at row 2 (rule 1): rule 1's
    assert agree([(I, A, 0, None, -1), (O, A, 0, None, -1), (F, R, 1, None, None)], keyed=False)["error"] == [PH.NO_OPEN]
    # a nil :invoke :add repaired by its :ok's value
    assert agree([(I, A, 0, None, None), (O, A, 0, None, 3)], keyed=False)["error"] == [None]
    # exactly INT64_MAX, and one more
    big = [(I, A, 0, None, PH.I64_MAX - 1), (I, A, 1, None, 1)]
    assert agree(big, keyed=False)["error"] == [None]
    assert agree(big + [(I, A, 2, None, 1)], keyed=False)["error"] == [PH.SUM]
    # a nil add before the overflow point, and after it
    assert agree([(I, A, 3, None, None)] + big + [(I, A, 2, None, 1)], keyed=False)["error"] == [PH.ADD_NIL]
    assert agree(big + [(I, A, 2, None, 1), (I, A, 3, None, None)], keyed=False)["error"] == [PH.SUM]
