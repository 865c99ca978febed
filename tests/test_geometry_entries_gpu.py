"""Which per-geometry-step entries invalidate the fields `ofdft_hessian_vector` keeps for reuse_density = 1, on
the fcc-Al 16^3 case of the force-constant tests with the six-term set of tests/test_hvp_gpu.py: after a product with
reuse_density=False one geometry entry runs, then the product is asked again with reuse_density=True.  The first-order ion entries
leave the fields alone (they live in workspaces of their own names), so the product comes back bit for bit; every second-order
entry and `ofdft_stress` clear them, so the product is refused with OFDFT_ESTATE (-3).  No tolerance anywhere: equal bits or a
refusal.  The same file pins the table-shape check of the seven ion wrappers, which runs before the engine is touched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fc_cases
import hvp_cases
from professad_amd import _native as N
from professad_amd import ions
from professad_amd.engine import Engine

DEV = 'cuda:0'
SIX = ('hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c')

_CASE = {}


def case():
    """inputs of the a16 case, made once and shared, never written"""
    if not _CASE:
        box, shape, frac, den, raw, k_max = fc_cases.make_inputs('a16')
        tab = ions.recpot_table(raw, k_max)
        _CASE.update(box=box, shape=shape, frac=frac, den=den, w=hvp_cases.direction(den.shape), species=[(frac, tab)],
                     z=np.full(frac.shape[0], float(tab[2])))
    return _CASE


def _strain_hessian_entry(eng, den):
    """ofdft_strain_hessian itself: `Engine.strain_hessian` goes on to a product of its own for the pointwise terms (den, den,
    reuse_density=False), which retains the fields of the same density again and would hide what the entry did"""
    buf = (C.c_double * (N.NTERMS * 81))()
    eng._check(eng.lib.ofdft_strain_hessian(eng._ctx, C.c_void_p(den.data_ptr()), buf, eng._stream()), 'ofdft_strain_hessian')


KEEPS = {
    'ionic_potential': lambda e, c, den: ions.ionic_potential(e, c['box'], c['species']),
    'ion_electron_forces': lambda e, c, den: ions.ion_electron_forces(e, c['box'], den, c['species']),
    'ion_electron_stress': lambda e, c, den: ions.ion_electron_stress(e, c['box'], den, c['species']),
    'ion_ion_direct': lambda e, c, den: ions.ion_ion(e, c['box'], c['frac'], c['z']),
    'ion_ion_cells': lambda e, c, den: ions.ion_ion(e, c['box'], c['frac'], c['z'], method='cells'),
}
CLEARS = {
    'stress': lambda e, c, den: e.stress(den),
    'ionic_potential_gradient': lambda e, c, den: ions.ionic_potential_gradient(e, c['box'], c['species'], 1),
    'ion_electron_curvature': lambda e, c, den: ions.ion_electron_curvature(e, c['box'], den, c['species']),
    'ion_ion_hessian': lambda e, c, den: ions.ion_ion_hessian(e, c['box'], c['frac'], c['z'], [0, 2]),
    'potential_strain_gradient': lambda e, c, den: e.potential_strain_gradient(den),
    'ionic_potential_strain_gradient': lambda e, c, den: ions.ionic_potential_strain_gradient(e, c['box'], c['species']),
    'strain_hessian': lambda e, c, den: _strain_hessian_entry(e, den),
    'ion_electron_strain_hessian': lambda e, c, den: ions.ion_electron_strain_hessian(e, c['box'], den, c['species']),
    'ion_ion_strain_hessian': lambda e, c, den: ions.ion_ion_strain_hessian(e, c['box'], c['frac'], c['z']),
}


def _product_then(entry):
    c = case()
    eng = Engine(c['shape'], DEV).set_cell(c['box']).set_terms(list(SIX))
    den = torch.as_tensor(c['den'], dtype=torch.double, device=DEV)
    w = torch.as_tensor(c['w'], dtype=torch.double, device=DEV)
    first = eng.hessian_vector(den, w, reuse_density=False).clone()
    entry(eng, c, den)
    return eng, den, w, first


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KEEPS))
def test_first_order_ion_entries_leave_the_retained_fields(name):
    eng, den, w, first = _product_then(KEEPS[name])
    again = eng.hessian_vector(den, w, reuse_density=True)
    eng.close()
    assert torch.equal(again, first)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CLEARS))
def test_second_order_entries_and_the_stress_clear_the_retained_fields(name):
    eng, den, w, _first = _product_then(CLEARS[name])
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(den, w, reuse_density=True)
    eng.close()


class _Untouched:
    """stands for the engine: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError('the engine was used (%s) before the tables were checked' % name)


@pytest.mark.parametrize('call', [
    lambda e, sp: ions.ionic_potential(e, None, sp),
    lambda e, sp: ions.ion_electron_forces(e, None, None, sp),
    lambda e, sp: ions.ion_electron_stress(e, None, None, sp),
    lambda e, sp: ions.ionic_potential_gradient(e, None, sp, 1),      # (an ion of the faulty species: this entry sends one species)
    lambda e, sp: ions.ion_electron_curvature(e, None, None, sp),
    lambda e, sp: ions.ionic_potential_strain_gradient(e, None, sp),
    lambda e, sp: ions.ion_electron_strain_hessian(e, None, None, sp),
], ids=['ionic_potential', 'ion_electron_forces', 'ion_electron_stress', 'ionic_potential_gradient', 'ion_electron_curvature',
        'ionic_potential_strain_gradient', 'ion_electron_strain_hessian'])
def test_ion_wrappers_refuse_tables_of_unequal_length_before_any_device_call(call):
    """C reads `ks.size` entries of both tables: a shorter v would be read past its end.  The second species carries the fault, so
    the check covers the whole list before the first species is sent."""
    ks = np.linspace(0.0, 4.0, 9)
    good, bad = (np.zeros((1, 3)), (ks, np.ones(9), 3.0)), (np.zeros((2, 3)), (ks, np.ones(8), 3.0))
    with pytest.raises(ValueError, match='equal length'):
        call(_Untouched(), [good, bad])
