"""Terminations and done codes at their thresholds: the device against the oracle on the lattice of tests/termination_util.py (the very
cases tests/test_termination_twin.py holds to account on the CPU), for every family and kernel form.

Per (family, form) every lattice of the family is one handle with as many envs as it has cases (at most 96; singlecombat's altitude
lattice has 70, a ragged last workgroup) and a chain of three teacher-forced steps: the decision and the two steps after it (the
auto-reset observation, current_step restarting at 1 and the Overload gate closed again after an episode end; the die_flag latch, the
frozen observation and the team mean after a partial death); the four missile tasks add 40-step chains for SafeReturn's missile clause.
`done`, the whole info row from the device buffers -- and for the altitude
lattice also the packed host word --, status, die_flag, bloods, cur_step and ticks must be equal; rewards and observations are held to
the family's existing teacher-forced bounds. Every case is at least five one-step bounds away from every threshold on the oracle's
side, so a decision that differs is a wrong comparison, not rounding. Each test prints, per threshold, the closest case on either
side as a multiple of the bound it was chosen against.

Above 1024 workgroups the launcher picks other builds of the munition, NvN and heading kernels (test_gpu_parity.py::
test_large_grid_kernel_variants_match_small_grid); the second test plays one lattice of each of those families as the first envs of a
70 000-aircraft handle."""
import pytest

import termination_util as T

pytestmark = pytest.mark.gpu

CASES = [(fam, form) for fam, F in T.FAMILIES.items() for form in F["forms"]]
IDS = [fam.replace(" ", "_") + "".join(f"-{k[10:].lower()}{v}" for k, v in form.items()) for fam, form in CASES]


@pytest.fixture(scope="module")
def ix(pkg):
    return T.field_index(pkg)


@pytest.mark.parametrize("fam,form", CASES, ids=IDS)
def test_terminations_match_the_oracle_at_their_thresholds(pkg, oracle, ix, monkeypatch, fam, form):
    for k, v in form.items():
        monkeypatch.setenv(k, v)        # ac_create reads the pin per handle
    lats = [T.lattice(pkg, oracle, ix, fam, key) for key in T.configs(fam)]
    name = ", ".join(f"{k}={v}" for k, v in form.items()) or "default form"
    for lat in lats:
        side = T.DeviceSide(pkg, lat)
        try:
            T.compare(lat, side, form=name, host_words=lat.key == "alt")
        finally:
            side.close()
    cov = T.coverage(lats)              # (compare() walks every case of every lattice: nothing is left out of the comparison)
    T.print_coverage(f"{fam}, {name}: every decision, done code and reset equal to the oracle's", cov)


LARGE = {"singlecombat_shoot": "g1", "singlecombat_dodge_missile": "alt", "scenario1": "g1", "scenario_nvn 2v2": "g1", "multiplecombat 2v2": "g1", "heading": "g1"}


@pytest.mark.parametrize("fam", list(LARGE), ids=[f.replace(" ", "_") for f in LARGE])
def test_large_grid_variants_decide_like_the_oracle(pkg, oracle, ix, fam):
    lat = T.lattice(pkg, oracle, ix, fam, LARGE[fam])
    side = T.DeviceSide(pkg, lat, envs=70000 // lat.A)
    try:
        T.compare(lat, side, form="large grid", host_words=True)
    finally:
        side.close()
    T.print_coverage(f"{fam} [{lat.key}], large grid: every decision, done code and reset equal to the oracle's", T.coverage([lat]))
