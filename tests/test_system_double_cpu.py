"""CPU tests of tests/system_double.py, the numpy double that tests/test_dropin_gradients_gpu.py and tests/test_ion_species_gpu.py
compare the drop-in layer with: the synthetic second recpot table carries the charge it was built for, both branches of the table
clamp are populated on every grid those files use, the double's stresses and forces are the derivatives of its own energies
(central differences on one tiny triclinic grid), and the comparison helpers reject a perturbed double.  No GPU anywhere; every test
prints its figures as `MEASURE ...` before it asserts.
"""
import numpy as np
import pytest

import spectral_check as sc
import system_double as SD
from oracle import ions as oi
from professad_amd import synth
from professad_amd.ions import recpot_table

# Central differences at the step and bound of tests/test_second_order_doubles_cpu.py: h = 1e-4 (bohr for positions, plain number
# for strains), truncation h^2 |f'''| / 6 -- 1e-7 of the quantity's maximum; an error in a closed form is of order one.
FD_STEP = 1e-4
FD_BOUND = 1e-7

TINY = ((9, 8, 10), 'tri')
# every (shape, cell) of the two GPU files
GPU_GRIDS = [((16, 8, 32), 'ortho'), ((27, 35, 33), 'tri'), ((48, 16, 32), 'tri'), ((16, 16, 32), 'ortho')]


def make_cell(shape, kind):
    """test_extent_matrix_gpu.make_cell (that module needs a device to import its engine; the recipe is two lines)"""
    if kind == 'ortho':
        return np.diag([7.6 * s / 32.0 * (1.0 + 0.1 * i) for i, s in enumerate(shape)])
    return synth.triclinic_cell(1.0) * (np.asarray(shape, dtype=float)[:, None] / 32.0)


def tiny_cell():
    """twice the matrix recipe (0.48 bohr per step): about 2.4 electrons, so that round(N_e) of WGC99 and vWGTF is not zero"""
    return 2.0 * make_cell(*TINY)


def tiny_inputs():
    shape, kind = TINY
    box = tiny_cell()
    den, vext, _chi = sc.full_spectrum_inputs(shape, 77)
    rng = np.random.default_rng(5)
    species = [(rng.random((2, 3)) * 1.6 - 0.3, SD.golden_recpot()), (rng.random((3, 3)) * 1.6 - 0.3, SD.second_recpot()[:2])]
    return box, den, vext, species


def test_make_cell_is_the_recipe_of_the_extent_matrix():
    import test_extent_matrix_gpu as M
    for shape, kind in GPU_GRIDS:
        assert np.array_equal(make_cell(shape, kind), M.make_cell(shape, kind))


def test_second_recpot_differs_from_the_golden_table_and_carries_its_charge():
    raw, k_max, z = SD.second_recpot()
    graw, gk = SD.golden_recpot()
    gz = recpot_table(graw, gk)[2]
    ks, v, got = recpot_table(raw, k_max)
    print('MEASURE second recpot: %d points, k_max %.1f, z %d (golden: %d points, k_max %.4f, z %d)' % (raw.size, k_max, got, graw.size, gk, gz))
    assert got == z and isinstance(got, int)
    assert oi.recpot_table(raw, k_max)[2] == z
    assert raw.size != graw.size and k_max != gk and z != gz
    # smooth: with the Coulomb tail added the table is continuous at k -> 0 and its second differences stay small
    assert abs(v[1] - v[0]) <= 1e-4 * abs(v[0])
    assert np.abs(np.diff(v, 2)).max() <= 1e-3 * np.abs(v).max()
    # one more unit of charge in the Coulomb part: the charge moves by one, the smooth part does not
    k2, v2, z2 = recpot_table(SD.charge_off_by_one(raw, k_max), k_max)
    assert z2 == z + 1 and np.allclose(v2, v, rtol=1e-10, atol=0)    # (4 pi / dk^2 = 3.7e5 cancels at the first points)


@pytest.mark.parametrize('shape,kind', GPU_GRIDS + [TINY], ids=lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else x)
def test_both_branches_of_the_table_clamp_are_populated(shape, kind):
    """beyond the end of the second table and inside it; the golden table (k_max = 30) covers every grid"""
    box = tiny_cell() if (shape, kind) == TINY else make_cell(shape, kind)
    inside, beyond = SD.clamp_census(box, shape, SD.SECOND_KMAX)
    g_inside, g_beyond = SD.clamp_census(box, shape, SD.golden_recpot()[1])
    print('MEASURE clamp %s %s: second table %d inside / %d beyond, golden table %d / %d' % (shape, kind, inside, beyond, g_inside, g_beyond))
    assert inside >= 8 and beyond >= 8
    assert g_inside >= 8
    # ... and the clamp matters: the potential of the clamped table differs from the one of a table that is not cut
    raw, k_max, _z = SD.second_recpot()
    kabs = np.sqrt(SD.cf.recip(box, shape)[3])
    vk = oi.recpot_on_grid(raw, k_max, kabs)
    ks, y, z = oi.recpot_table(raw, k_max)
    far = kabs > k_max
    assert np.allclose(vk[far], y[-1] - 4 * np.pi * z / kabs[far] ** 2, rtol=1e-14, atol=0)


def _strained(box, i, j, h):
    eps = np.zeros((3, 3))
    eps[i, j] += h / 2
    eps[j, i] += h / 2
    return box @ (np.eye(3) + eps)


def test_stress_of_the_double_is_the_strain_derivative_of_its_energy():
    """per callable and for the total (functionals + the ion-electron energy with v_ext rebuilt from the species at fixed fractional
    coordinates): sigma_ij = (1 / vol) dE / d eps_ij at fixed electron number, the density grid scaled as 1 / volume"""
    box, den, _vext, species = tiny_inputs()
    vol = abs(np.linalg.det(box))

    def energies(b):
        n = den * vol / abs(np.linalg.det(b))
        out = {k: e[0] for k, e in SD.evaluate(b, n).items()}
        out['ions'] = SD.species_energy(b, n, species)
        out['total'] = out['sum'] + out['ions']
        return out

    sig = {k: e[2] for k, e in SD.evaluate(box, den).items()}
    sig['ions'] = SD.species_stress(box, den, species)
    sig['total'] = sig['sum'] + sig['ions']
    fd = {k: np.zeros((3, 3)) for k in sig}
    for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)):
        Ep, Em = energies(_strained(box, i, j, FD_STEP)), energies(_strained(box, i, j, -FD_STEP))
        for k in sig:
            fd[k][i, j] = fd[k][j, i] = (Ep[k] - Em[k]) / (2 * FD_STEP) / vol
    worst = {k: SD.rel(fd[k], sig[k]) for k in sig}
    for k, e in worst.items():
        print('MEASURE strain difference %-26s %.2e of max|sigma| = %.3e' % (k, e, np.abs(sig[k]).max()))
    bad = {k: e for k, e in worst.items() if not e <= FD_BOUND}
    assert not bad, bad


def test_forces_of_the_double_are_the_position_derivative_of_its_energy():
    box, den, _vext, species = tiny_inputs()
    inv = np.linalg.inv(box)
    F = SD.species_forces(box, den, species)
    scale = max(np.abs(f).max() for f in F)
    worst = 0.0
    for s, (frac, tab) in enumerate(species):
        for a in range(frac.shape[0]):
            for j in range(3):
                E = {}
                for sign in (+1, -1):
                    cart = frac @ box
                    cart[a, j] += sign * FD_STEP
                    moved = list(species)
                    moved[s] = (cart @ inv, tab)
                    E[sign] = SD.species_energy(box, den, moved)
                worst = max(worst, abs(-(E[+1] - E[-1]) / (2 * FD_STEP) - F[s][a, j]))
    print('MEASURE position difference: %.2e of max|F| = %.3e' % (worst / scale, scale))
    assert worst <= FD_BOUND * scale
    # PME forces are the derivative of the PME energy too (order 6 on this grid: below its smallest extent)
    Fp = SD.species_forces(box, den, species, 6)
    frac, tab = species[1]
    E = {}
    for sign in (+1, -1):
        cart = frac @ box
        cart[2, 1] += sign * FD_STEP
        E[sign] = SD.species_energy(box, den, [species[0], (cart @ inv, tab)], 6)
    e = abs(-(E[+1] - E[-1]) / (2 * FD_STEP) - Fp[1][2, 1]) / np.abs(Fp[1]).max()
    print('MEASURE position difference, PME 6: %.2e' % e)
    assert e <= FD_BOUND


def test_ion_routines_are_linear_in_the_species():
    box, den, _vext, species = tiny_inputs()
    v = SD.species_potential(box, den.shape, species)
    assert np.array_equal(v, SD.species_potential(box, den.shape, species[:1]) + SD.species_potential(box, den.shape, species[1:]))
    s = SD.species_stress(box, den, species)
    assert SD.rel(SD.species_stress(box, den, species[::-1]), s) <= 1e-14
    F, Fr = SD.species_forces(box, den, species), SD.species_forces(box, den, species[::-1])
    assert np.array_equal(F[0], Fr[1]) and np.array_equal(F[1], Fr[0])


# ----------------------------------------------------------------------------------------------------- the helpers bite
def test_comparison_helpers_reject_a_perturbed_double():
    """the unperturbed double stands in for the engine; the perturbed one for the reference value it is checked against"""
    box, den, vext, species = tiny_inputs()
    ev = SD.evaluate(box, den, ['Hartree', 'WGC99', 'PerdewBurkeErnzerhof'], vext)
    E, v, sig = ev['sum']
    SD.check_field(v, v, 'same', E, E)
    SD.check_stress(sig, sig)
    # one entry of the potential off by 1e-9 relative
    k = np.unravel_index(np.argmax(np.abs(v)), v.shape)
    vp = v.copy()
    vp[k] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        SD.check_field(v, vp, 'one entry')
    # the energy off by 1e-12 relative (E_TOL is 1e-13)
    with pytest.raises(AssertionError):
        SD.check_field(v, v, 'energy', E, E * (1 + 1e-12) if abs(E) >= 1 else E + 1e-12)
    # one stress component scaled by 1 + 1e-8
    sp = sig.copy()
    i = np.unravel_index(np.argmax(np.abs(sig)), sig.shape)
    sp[i] *= 1 + 1e-8
    with pytest.raises(AssertionError):
        SD.check_stress(sig, sp)
    # ion routines: one entry of v_ext, one stress component, one force component, and a species' charge off by one
    vi, Fi, si = SD.species_potential(box, den.shape, species), SD.species_forces(box, den, species), SD.species_stress(box, den, species)
    SD.check_ion_potential(vi, vi)
    SD.check_forces(Fi, Fi)
    SD.check_stress(si, si, SD.ION_SIG_RTOL)
    k = np.unravel_index(np.argmax(np.abs(vi)), vi.shape)
    vp = vi.copy()
    vp[k] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        SD.check_ion_potential(vi, vp)
    sp = si.copy()
    sp[np.unravel_index(np.argmax(np.abs(si)), si.shape)] *= 1 + 1e-8
    with pytest.raises(AssertionError):
        SD.check_stress(si, sp, SD.ION_SIG_RTOL)
    Fp = [f.copy() for f in Fi]
    Fp[1][np.unravel_index(np.argmax(np.abs(Fi[1])), Fi[1].shape)] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        SD.check_forces(Fi, Fp)
    raw, k_max = species[1][1]
    wrong = [species[0], (species[1][0], (SD.charge_off_by_one(raw, k_max), k_max))]
    assert SD.tables(wrong)[1][1][2] == SD.SECOND_Z + 1
    with pytest.raises(AssertionError):
        SD.check_ion_potential(vi, SD.species_potential(box, den.shape, wrong))
    with pytest.raises(AssertionError):
        SD.check_forces(Fi, SD.species_forces(box, den, wrong))
    with pytest.raises(AssertionError):
        SD.check_stress(si, SD.species_stress(box, den, wrong), SD.ION_SIG_RTOL)
    # forces handed back in the other species' slot
    with pytest.raises(AssertionError):
        SD.check_forces(Fi[::-1], Fi)
