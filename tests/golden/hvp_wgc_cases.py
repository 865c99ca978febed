"""Cases and term sets of the WGC99 Hessian-vector goldens (make_golden_hvp_wgc.py and make_golden_tn_wgc.py write them,
tests/test_hvp_wgc_cpu.py, tests/test_hvp_wgc_gpu.py and tests/test_tn_wgc_gpu.py read them): the grids, direction and seeds of
hvp_cases.py; the truncated-Newton cases are those of tn_cases.py with cfg3w's term set.  The ground state, response and counts
are kept for GS_CASES only: on g17r the reference-driven line search stalls at |g|_2 = 9.8e-9, so that case has the chi-space
product and gradient alone (its chirp-z path is covered by the product goldens)."""
import hvp_cases
import tn_cases

CASES = hvp_cases.CASES                 # g16r, g17r, g18t, g16d
TN_CASES = tn_cases.CASES               # g16r, g17r, g18t
GS_CASES = ['g16r', 'g18t']
# golden key -> engine term names (WGC99's parameters are the defaults: alpha, beta = (5 +- sqrt 5) / 6, gamma = 2.7, kappa = 1)
TERMS = {'wgc99_nl': ('wgc99_nl',), 'wgc99': ('tf', 'vw', 'wgc99_nl')}
# the term set of the headline benchmark, and the same with Perdew-Zunger LDA
CFG3W = ('ion_electron', 'hartree', 'tf', 'vw', 'wgc99_nl', 'pbe_x', 'pbe_c')
CFG2W = ('ion_electron', 'hartree', 'tf', 'vw', 'wgc99_nl', 'lda_x', 'pz_c')
SETS = {'cfg3w': CFG3W, 'cfg2w': CFG2W}
KEYS = {**TERMS, **SETS}
# mean(den) vol must stay this far from a half-integer: round(N) is a constant of the differentiation only away from its jumps
HALF_INTEGER_MARGIN = 0.1

make_inputs = hvp_cases.make_inputs
direction = hvp_cases.direction
