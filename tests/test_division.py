"""The smoother divides by the diagonal with a reciprocal + one Markstein
correction (kernels.hip div_diag).  This checks on the host, with the same
instruction sequence (fma from libm), that it is bitwise IEEE division for
every diagonal the solver uses and for random divisors -- on a domain: finite
numerators that are zero or at least 2^-969 in magnitude.  The proof needs the
remainder a - q0 d exact; it is a multiple of 2^(e(q0) + e(d) - 104), so it can
underflow once e(q0) + e(d) < -970, which e(a) >= -969 excludes and e(a) = -970
does not (tools/check_division.c).  Below, both forms of div_diag are within one
ulp; a = +-Inf gives NaN.

Measured (60 diagonals; mismatches are the same numerators in POSD, the general
form and the general form with -d, each exactly one ulp): none in any band from
2^-969 to the largest finite double, and none yet in the binades just below --
a rounded remainder only matters where it tips the last rounding, which gets
likelier by a factor of two per binade.  Per binade, of 6 M numerators:
2^-1000 and above 0, 2^-1003 4, 2^-1006 28, 2^-1010 442, 2^-1015 19070 (0.3 %),
2^-1020 621384 (10 %); over [2^-1022, 2^-969) 9264 of 1.2 M, subnormal
numerators 14181 of 1.2 M.  So 2^-969 is the proven bound, and a field has to
decay to about 1e-302 before a mismatch is seen."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_markstein_division_is_correctly_rounded(tmp_path):
    exe = tmp_path / "check_division"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tools", "check_division.c"), "-lm"], check=True)
    out = subprocess.run([str(exe), "300000", "20000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "mismatches 0" in out.stdout


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = tmp_path_factory.mktemp("division") / "check_division"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(ROOT, "tools", "check_division.c"), "-lm"], check=True)
    return str(exe)


def run_range(tool, elo, ehi, per=20000):
    """-> {form: (mismatches, max ulp)}, tests"""
    out = subprocess.run([tool, "range", str(elo), str(ehi), str(per)], capture_output=True,
                         text=True, check=True).stdout
    print(out.strip())
    forms = {m[0]: (int(m[1]), int(m[2]))
             for m in re.findall(r"(posd|general|general_negd) mismatches (\d+) max_ulp (\d+)", out)}
    assert set(forms) == {"posd", "general", "general_negd"}, out
    tests = int(re.search(r"tests (\d+)", out).group(1))
    assert tests == 60 * per, out
    return forms, tests


THRESHOLD = -969   # |a| >= 2^-969: the remainder cannot underflow
BANDS = [(THRESHOLD, -960), (-959, -900), (-899, -500), (-499, -201), (-200, 200), (201, 600),
         (601, 1000), (1001, 1022), (1023, 1023)]


@pytest.mark.parametrize("elo,ehi", BANDS)
def test_division_is_bitwise_from_the_threshold_to_the_largest_double(tool, elo, ehi):
    forms, _ = run_range(tool, elo, ehi)
    assert forms == {"posd": (0, 0), "general": (0, 0), "general_negd": (0, 0)}


@pytest.mark.parametrize("elo,ehi", [(-1022, -970), (-1023, -1023)],
                         ids=["normal_below", "subnormal"])
def test_below_the_threshold_every_mismatch_is_one_ulp(tool, elo, ehi):
    """What the documented domain excludes: there are mismatches, each exactly
    one ulp, the same in both forms."""
    forms, tests = run_range(tool, elo, ehi)
    for form, (bad, worst) in forms.items():
        assert 0 < bad < tests and worst == 1, (form, bad, worst)
    assert len({bad for bad, _ in forms.values()}) == 1, forms


def test_the_binades_just_below_the_threshold_are_within_one_ulp(tool):
    """[2^-1000, 2^-969): outside the proof, no mismatch measured; only the one
    ulp is asserted."""
    forms, _ = run_range(tool, -1000, -970)
    assert all(worst <= 1 for _, worst in forms.values()), forms


def test_zero_and_nan_agree_and_inf_gives_nan(tool):
    out = subprocess.run([tool, "special"], capture_output=True, text=True, check=True).stdout
    m = re.search(r"divisors (\d+), zero mismatches (\d+), nan mismatches (\d+), "
                  r"inf results that are not NaN (\d+)", out)
    assert m, out
    assert [int(x) for x in m.groups()] == [60, 0, 0, 0], out
