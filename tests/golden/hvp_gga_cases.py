"""Cases and term sets of the PBE Hessian-vector goldens (make_golden_hvp_gga.py and make_golden_tn_gga.py write them,
tests/test_hvp_gga_cpu.py, tests/test_hvp_gga_gpu.py and tests/test_tn_gga_gpu.py read them): the grids, direction and seeds of
hvp_cases.py; the truncated-Newton cases are those of tn_cases.py with cfg3's term set."""
import hvp_cases
import tn_cases

CASES = hvp_cases.CASES                 # g16r, g17r, g18t, g16d
TN_CASES = tn_cases.CASES               # g16r, g17r, g18t
# golden key -> engine term names
TERMS = {'pbe_x': ('pbe_x',), 'pbe_c': ('pbe_c',), 'pbe': ('pbe_x', 'pbe_c')}
# Wang-Teter + PBE: the term set the reference checks against PROFESS and the one of the headline benchmark
CFG3 = (('ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'pbe_x', 'pbe_c'), 5 / 6, 5 / 6)
SETS = {'cfg3': CFG3}

make_inputs = hvp_cases.make_inputs
direction = hvp_cases.direction
