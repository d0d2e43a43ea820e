"""The records and the checker of dr_fr_raw_selftest (tests/law_images.py, second half) without a GPU: every built image meets the contract
of the operations its record names, each operation's records reach BOTH ends of every bound its header documents (asserted on the
built inputs, so that a pool that silently misses an edge fails here and not on the GPU), the checker accepts the header's own
arithmetic in Python integers and rejects a limb changed by one, a value off by p where the very integer is promised, a limb one
unit outside its class and a wrong flag.

fr29.hip.h's products are montmul9x29_asm / montsqr9x29_asm / montmul2_9x29_asm, gfx950 assembly: there is no host build of the field to
run under a sanitizer, and none is loaded into Python.  tests/test_montmul_gen.py interprets the generated text instruction by
instruction; what the device makes of it at these bounds is tests/test_gpu_fr_raw.py."""
import law_images as L

P, M29 = L.FR_P, L.M29


def _with(op):
    return [r for r in L.fr_records() if op in r.ops]


def _maxabs(image):
    return max(abs(x) for x in image)


def test_every_record_meets_the_contract_of_what_it_names():
    records = L.fr_records()
    assert 300 < len(records) < 1000 and len({r.what for r in records}) == len(records)
    assert {op for r in records for op in r.ops} == set(L.FR_LIMB_SLOTS + L.FR_WORD_SLOTS + L.FR_FLAGS)
    spread = L.fr_spread(65)                               # what the calls of 1, 64 and 65 records take
    assert len(spread) == len({id(r) for r in spread}) == 65 and {op for r in spread[:64] for op in r.ops} == {op for r in records for op in r.ops}
    for r in records:
        va, vb = L.fr_value(r.a), L.fr_value(r.b)
        if "mul" in r.ops:                                # fr29.hip.h:15: 2^30 x 2^29, or 1.6 * 2^29 twice
            assert _maxabs(r.a) * _maxabs(r.b) <= L.FR_MUL_WIDE * L.FR_MUL_NARROW or max(_maxabs(r.a), _maxabs(r.b)) <= L.FR_MUL_BOTH, r.what
        if "sqr" in r.ops:
            assert _maxabs(r.a) <= L.FR_MUL_BOTH and va * va <= L.FR_MUL_VALUE, r.what
        if "mul2" in r.ops:
            assert max(map(_maxabs, (r.a, r.b, r.c, r.d))) <= L.FR_MUL2_LIMB and abs(va * vb + L.fr_value(r.c) * L.fr_value(r.d)) <= L.FR_MUL_VALUE, r.what
        if "carry" in r.ops or "reduce_small" in r.ops:
            assert _maxabs(r.a[:8]) <= L.FR_CARRY_LIMB and abs(r.a[8]) <= (1 << 31) - 8, r.what
        if "reduce_small" in r.ops:
            assert abs(va) < L.FR_REDUCE_VALUE, r.what
        if "carry_u" in r.ops or "sub_3p" in r.ops:
            assert all(0 <= x <= L.FR_CARRY_U_LIMB for x in r.a[:8]) and abs(r.a[8]) < 1 << 30, r.what
        if r.ops & {"canon29", "repack", "inv", "fs_to_std", "to_mont256"}:
            assert abs(va) <= L.FR_CANON_VALUE and _maxabs(r.a) <= L.FR_CARRY_LIMB, r.what
            assert abs(va) < L.FR_CANON_VALUE or va == -L.FR_CANON_VALUE, r.what                  # -8 p itself: + 8 p makes it 0
        if "to_mont256" in r.ops:
            assert _maxabs(r.a) <= L.FR_MUL_WIDE, r.what
        if "canon29_small" in r.ops:
            assert -P < va < 3 * P, r.what
        if "is_zero" in r.ops:
            assert abs(va) < L.FR_ZERO_VALUE or va in (L.FR_ZERO_VALUE, -L.FR_ZERO_VALUE), r.what
        if "equal" in r.ops:
            assert abs(va - vb) <= L.FR_ZERO_VALUE and all(abs(x - y) < 1 << 31 for x, y in zip(r.a, r.b)), r.what
        if "aA_b" in r.ops:
            for image in (r.a, r.b):                     # curve.hip.h:66: a product of normal operands
                assert all(0 <= x <= M29 for x in image[:8]) and L.FR_PRODUCT_LO <= L.fr_value(image) <= L.FR_PRODUCT_HI, r.what


def test_mul_sqr_and_mul2_reach_both_ends_of_their_bounds():
    mul = _with("mul")
    near = lambda v: L.FR_MUL_VALUE - (35 * P << L.FR_TOP) < abs(v) <= L.FR_MUL_VALUE         # within one unit of the top limbs
    # the limb bound at its largest, 2^30 against 2^29 in either order and 1.6 * 2^29 twice, in every arrangement of signs ...
    for wide, narrow in ((L.FR_MUL_WIDE, L.FR_MUL_NARROW), (L.FR_MUL_NARROW, L.FR_MUL_WIDE), (L.FR_MUL_BOTH, L.FR_MUL_BOTH)):
        signs = set()
        for r in mul:
            if all(abs(x) == wide for x in r.a[:8]) and all(abs(x) == narrow for x in r.b[:8]) and near(L.fr_value(r.a) * L.fr_value(r.b)):
                signs.add((r.a[0] > 0, r.a[1] > 0, r.b[0] > 0, r.b[1] > 0, L.fr_value(r.a) > 0, L.fr_value(r.b) > 0))
        assert {s[:4] for s in signs} >= {(x, x, y, y) for x in (True, False) for y in (True, False)}, (wide, narrow)    # nine products of one sign
        assert any(s[0] != s[1] for s in signs) and any(s[2] != s[3] for s in signs)                                       # and mixed columns
        assert {s[4:] for s in signs} == {(x, y) for x in (True, False) for y in (True, False)} or wide == L.FR_MUL_NARROW
    assert any(abs(x) == L.FR_MUL_WIDE for r in mul for x in r.a[8:])                                                  # the top limb at 2^30 too
    # ... one pair beyond 35 p^2, and products of either sign there
    beyond = [L.fr_value(r.a) * L.fr_value(r.b) for r in mul if abs(L.fr_value(r.a) * L.fr_value(r.b)) > L.FR_MUL_VALUE]
    assert beyond and min(beyond) < 0 < max(beyond)
    sqr = _with("sqr")
    for first, second in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        assert any(r.a[0] == first * L.FR_MUL_BOTH and r.a[1] == second * L.FR_MUL_BOTH and near(L.fr_value(r.a) ** 2) for r in sqr)
    mul2 = _with("mul2")
    assert all(abs(x) == M29 for r in mul2 for image in (r.a, r.b, r.c, r.d) for x in image[:8])
    kinds = set()
    for r in mul2:
        ab, cd = L.fr_value(r.a) * L.fr_value(r.b), L.fr_value(r.c) * L.fr_value(r.d)
        assert L.FR_MUL_VALUE - (40 * P << L.FR_TOP) < abs(ab + cd) <= L.FR_MUL_VALUE, r.what
        kinds.add(((ab > 0) == (cd > 0), ab + cd > 0))
    assert kinds == {(x, y) for x in (True, False) for y in (True, False)}       # the products of the same and of opposite signs, both totals
    assert {tuple(x > 0 for x in (r.a[0], r.b[0], r.c[0], r.d[0])) for r in mul2} >= {(True,) * 4, (False,) * 4}


def test_the_carries_reach_the_32_bit_edges():
    carry = _with("carry")
    for pattern in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        assert any(r.a[0] == pattern[0] * L.FR_CARRY_LIMB and r.a[1] == pattern[1] * L.FR_CARRY_LIMB for r in carry)
    assert any(min(r.a) < 0 < max(r.a) and _maxabs(r.a) < L.FR_CARRY_LIMB for r in carry)
    # what the header said before ("limbs within int32") cannot be met: the first carry already overflows
    assert (1 << 31) - 1 + 3 >= 1 << 31
    cu = _with("carry_u")
    assert any(all(x == 7 * M29 for x in r.a[:8]) for r in cu) and any(all(x == L.FR_CARRY_U_LIMB for x in r.a[:8]) for r in cu)
    assert any(all(x == 0 for x in r.a) for r in cu)
    assert L.FR_CARRY_U_LIMB + 7 == (1 << 32) - 1 and (L.FR_CARRY_U_LIMB >> 29) == 7       # the largest carry still fits; one more would not
    sub = [L.fr_value(r.a, True) for r in _with("sub_3p")]
    assert any(0 < v < 6 * P for v in sub) and any(5 * P < v < 6 * P for v in sub) and any(v <= 0 for v in sub) and any(v >= 6 * P for v in sub)


def test_reduce_small_reaches_every_half_and_both_ends():
    values = [L.fr_value(r.a) for r in _with("reduce_small")]
    assert L.FR_REDUCE_VALUE - 1 in values and -(L.FR_REDUCE_VALUE - 1) in values
    for q in range(-30, 30):
        half = (2 * q + 1) * P // 2
        assert half in values and half + 1 in values, q                                     # the two integers beside (q + 1/2) p
        assert any(0 < half - v <= 8 << L.FR_TOP for v in values) and any(0 < v - half - 1 <= 8 << L.FR_TOP for v in values), q
    assert max(values) > 29 * P and min(values) < -29 * P
    forms = {("digits" if all(0 <= x <= M29 for x in r.a[:8]) else "big" if _maxabs(r.a) > 1 << 30 else "lazy") for r in _with("reduce_small")}
    assert forms == {"digits", "lazy", "big"}


def test_canon_inv_is_zero_and_equal_reach_their_cases():
    canon = {L.fr_value(r.a) for r in _with("canon29")}
    assert canon >= {k * P + v for k in range(-8, 8) for v in (0, 1, P - 1)}
    assert any(not all(0 <= x <= M29 for x in r.a[:8]) for r in _with("canon29"))            # not only carried images
    small = {L.fr_value(r.a) for r in _with("canon29_small")}
    assert small >= {k * P + v for k in range(-1, 3) for v in (0, 1, P - 1) if -P < k * P + v < 3 * P} | {-P + 1, 3 * P - 1}
    inv = {L.fr_value(r.a) for r in _with("inv")}
    assert inv >= {0, P, -P, 1, -1, 8 * P - 1, -8 * P + 1, 7 * P, -7 * P}
    zero = _with("is_zero")
    for k in range(-4, 5):
        assert any(L.fr_value(r.a) == k * P and not all(0 <= x <= M29 for x in r.a[:8]) for r in zero), k
    passing = set(range(5)) | set(range((1 << 29) - 4, 1 << 29))
    for d in passing:
        assert any(L.fr_value(r.a) % P and abs(L.fr_value(r.a)) < 4 * P and (r.a[0] & M29) == d for r in zero), d
    equal = [L.fr_value(r.a) - L.fr_value(r.b) for r in _with("equal")]
    assert set(equal) >= {k * P for k in range(-4, 5)} and any(v % P for v in equal)
    ends = {(L.fr_value(r.a), L.fr_value(r.b)) for r in _with("aA_b")}
    assert ends >= {(x, y) for x in (L.FR_PRODUCT_LO, L.FR_PRODUCT_HI) for y in (L.FR_PRODUCT_LO, L.FR_PRODUCT_HI)}
    assert any(all(x == M29 for x in r.a[:8] + r.b[:8]) for r in _with("bmaA_b"))            # six times 2^29 - 1 in every low limb


def test_checker_accepts_the_headers_arithmetic_and_rejects_what_is_wrong():
    records = L.fr_records()
    raw = b"".join(L.fr_model_words(r) for r in records)
    assert len(raw) == len(records) * L.FR_OUT_WORDS * 4 and len(L.pack_fr_records(records)) == len(records) * L.FR_IN_WORDS * 4
    results = L.unpack_fr_results(raw, len(records))
    assert L.check_fr_records(records, results) == []
    seen = set()
    for r, res in zip(records, results):
        for op in r.ops - seen:
            seen.add(op)
            wrong = {k: (list(v) if isinstance(v, list) else v) for k, v in res.items()}
            if op in L.FR_LIMB_SLOTS:
                wrong[op][4] += 1 if wrong[op][4] < M29 else -1                              # a limb changed by one
                bad = L.check_fr_record(r, wrong)
                assert len(bad) >= 1 and all(f"slot {op} " in b for b in bad) and any("limb 4 = " in b for b in bad), (op, bad)
                wrong[op] = list(res[op])
                wrong[op][0] = (1 << 29) if op not in ("aA_j",) else wrong[op][0] + 1          # a limb one unit outside its class
                wrong[op][1] -= 1 if op not in ("aA_j",) else 0                                # ... the value kept
                assert any(f"slot {op} " in b for b in L.check_fr_record(r, wrong)), op
                if op in ("carry", "carry_u", "sub_3p", "aA_b", "bmaA_b", "bmaA_j"):          # the very integer: off by p is not accepted
                    wrong[op] = [x + y for x, y in zip(res[op], L.fr_digits(P))]
                    assert any(f"slot {op} " in b and "has the value" in b for b in L.check_fr_record(r, wrong)), op
            elif op in L.FR_WORD_SLOTS:
                wrong[op] ^= 1 << 200
                assert any(op in b for b in L.check_fr_record(r, wrong)), op
            else:
                wrong[op] ^= 1
                assert any(op in b for b in L.check_fr_record(r, wrong)), op
    assert seen == set(L.FR_LIMB_SLOTS + L.FR_WORD_SLOTS + L.FR_FLAGS)
    # a product one unit of the top limb outside "normal" is outside, though congruent
    r = next(x for x in records if x.ops == {"mul"} and abs(L.fr_value(x.a) * L.fr_value(x.b)) <= L.FR_MUL_VALUE)
    res = dict(results[records.index(r)])
    res["mul"] = L.fr_digits(L.fr_value(res["mul"]) + 2 * P)
    assert any("outside its class normal" in b for b in L.check_fr_record(r, res))
    # beyond 35 p^2 the wider class holds, and not more
    r = next(x for x in records if x.what.startswith("mul beyond"))
    res = dict(results[records.index(r)])
    assert not L.FR_NORMAL.contains(res["mul"], 29) or abs(L.fr_value(r.a) * L.fr_value(r.b)) < 100 * P * P
    res["mul"] = L.fr_digits(L.fr_value(res["mul"]) + P)
    assert any("wide product" in b for b in L.check_fr_record(r, res))
