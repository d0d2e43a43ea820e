"""CPU: the signed 4-bit recoding of the fixed-schedule scalar multiplication (dot_ring_amd/csrc/wave_recode.hip.h), compiled for the host
as it is.  tests/native/wave_recode_check.cpp runs wave_recode<8>, <14> and <17> (the 256-bit curves, Ed448 / Curve448, P-521) on 0, 1,
2^(32 KW) - 1, the largest digit in every nibble (all 7s), a carry out of every nibble (all 8s), the group orders of the width and
their neighbours, and seeded random values: every digit in [-8, 7] and sum d 16^i + carry 16^(8 KW) = k; for 17 words and k < 2^521
the digits above window 130 are zero and no carry leaves."""
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref  # noqa: E402
import ed448_ref  # noqa: E402
import p256_ref  # noqa: E402
import p521_ref  # noqa: E402
import secp256k1_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = {8: [ed25519_ref.N, p256_ref.N, secp256k1_ref.N], 14: [ed448_ref.N], 17: [p521_ref.N]}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("wave_recode") / "wave_recode_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "wave_recode_check.cpp"), "-o", str(path)], check=True)
    return str(path)


def _scalars(kw):
    rng = random.Random(kw)
    nibbles = 8 * kw
    ks = [0, 1, 2**(32 * kw) - 1, int("7" * nibbles, 16), int("8" * nibbles, 16)]
    ks += [n + e for n in ORDERS[kw] for e in (-1, 0, 1)]
    ks += [rng.randrange(2**(32 * kw)) for _ in range(8)]
    if kw == 17:                                           # what the P-521 kernels are given: k < 2^521
        ks += [2**521 - 1, 2**520, int("7" * 130, 16) + (1 << 520), int("8" * 130, 16)] + [rng.randrange(2**521) for _ in range(8)]
    return ks


@pytest.mark.parametrize("kw", [8, 14, 17])
def test_digits_and_carry_sum_back_to_the_scalar(exe, kw):
    ks = _scalars(kw)
    proc = subprocess.run([exe], input="".join(f"{kw} {k:x}\n" for k in ks), capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    rows = [[int(x) for x in line.split()] for line in proc.stdout.splitlines()]
    assert len(rows) == len(ks)
    for k, row in zip(ks, rows):
        digits, carry = row[:-1], row[-1]
        assert len(digits) == 8 * kw and all(-8 <= x <= 7 for x in digits) and carry in (0, 1)
        assert sum(x * 16**i for i, x in enumerate(digits)) + carry * 16**(8 * kw) == k
        if kw == 17 and k < 2**521:                        # 131 windows and nothing leaves the top one
            assert digits[131:] == [0] * 5 and carry == 0
    assert any(row[-1] == 1 for row in rows) and any(row[-1] == 0 for row in rows)
