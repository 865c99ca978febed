"""Host-side checks of the measurement tooling (no GPU): the per-class byte model, the rocprofv3 classifier, the
reference pin of the bench workload and the worker launcher's refusal paths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench  # noqa: E402
import rocprof_summary  # noqa: E402


def test_every_kernel_class_of_the_committed_profile_is_classified_and_has_bytes():
    """the kernel names of the round-1 rocprofv3 table: each engine kernel maps to a class, each class that moves
    grid-sized data has an algorithmic-bytes entry, and the per-evaluation sum is DESIGN.md's 88C + 12R (13.5 GB; + 4C of WGC99 kernel tables in the counters)"""
    names = []
    with open(os.path.join(ROOT, 'profiles', 'r01_final_rocprof_serialised.md')) as fh:
        for line in fh:
            if line.startswith('| ') and not line.startswith('| kernel') and not line.startswith('|---'):
                names.append(line.split('|')[1].strip())
    assert len(names) > 15
    n, word = 256, 8
    cab = bench.class_alg_bytes('cfg3', n, word, 19.0)
    small = {'reduce', 'wgc_table'}
    seen = set()
    for nm in names:
        if any(f in nm for f in rocprof_summary.FOREIGN):
            continue
        c = rocprof_summary.klass(nm)
        assert c is not None, nm
        assert c in cab or c in small, (nm, c)
        seen.add(c)
    assert {'cpass_y', 'xfused_wgc', 'zpbe', 'zi_wgc', 'yderiv', 'xfused_div', 'zf_powers', 'zi_combine'} <= seen
    R, C = 8.0 * n ** 3, 16.0 * n * n * (n // 2 + 1)
    total = sum(v for k, v in cab.items() if k in seen)
    assert abs(total - (88 * C + 12 * R)) < 0.01 * total          # what the fused pipeline must move (kernel tables excluded)
    assert 13.0e9 < total < 14.0e9


def test_algorithmic_bytes_model_is_the_survey_contract():
    alg, R, C = bench.algorithmic_bytes(256, 'cfg3', 8)
    assert abs(alg - (23 * (R + 5 * C) + 25 * R)) < 1.0 and abs(alg - 22.0e9) < 0.05e9


def test_eval_roofline_fraction_is_formed_from_real_hbm_bytes_and_never_exceeds_one():
    """round-2 verdict: 22.0 GB of MODEL bytes / 2.7046 ms = 8.13 TB/s is not a roofline fraction.  The fraction comes from
    the measured (PMC) bytes, or from the per-class algorithmic bytes when no PMC file belongs to the build; the model figure
    is reported as a model-equivalent rate without a fraction"""
    alg, R, C = bench.algorithmic_bytes(256, 'cfg3', 8)
    cab = bench.class_alg_bytes('cfg3', 256, 8, 19.0)
    assert abs(cab['xfused_wgc'] - 12 * C) < 1.0           # kernel tables earn no algorithmic bytes
    class_bytes = sum(cab[k] for k in ('sum', 'chi_grad', 'cpass_y', 'xfused_lap', 'zf_density', 'yderiv', 'xfused_n', 'xfused_div',
                                       'xfused_wgc', 'zpbe', 'zf_powers', 'zi_wgc', 'zi_combine'))
    with_pmc = bench.eval_roofline_block(alg, 2.7046, 1, 14148066666.7, class_bytes)
    assert abs(with_pmc['achieved_GBs_per_gpu'] - 5231.1) < 1.0 and abs(with_pmc['frac'] - 0.6539) < 2e-4
    no_pmc = bench.eval_roofline_block(alg, 2.7046, 1, None, class_bytes)
    assert 0.60 < no_pmc['frac'] < 0.68 and 'algorithmic' in no_pmc['hbm_bytes_basis']
    for blk in (with_pmc, no_pmc):
        assert 'frac_of_peak' not in blk and blk['frac'] <= 1.0
        assert blk['model_equivalent_GBs_per_gpu'] > 8000.0        # the model rate may exceed the peak: hence no fraction for it
        assert not any('frac' in k for k in blk if k.startswith('model'))
    # per-GPU figures of a slab-decomposed run: every rank moves 1 / world of the class bytes
    two = bench.eval_roofline_block(alg, 2.7046, 2, None, class_bytes)
    assert abs(two['hbm_bytes_per_eval_per_gpu'] * 2 - class_bytes) < 1.0
    # even an impossibly fast step cannot produce a fraction above one without it being visible as such: the block carries
    # the bytes and the time it was formed from
    assert set(no_pmc) >= {'hbm_bytes_per_eval_per_gpu', 'hbm_bytes_basis', 'achieved_GBs_per_gpu', 'peak_GBs', 'frac', 'model_bytes_per_eval'}


def test_committed_bench_lines_of_this_round_carry_no_fraction_above_one():
    import glob
    files = glob.glob(os.path.join(ROOT, 'profiles', 'bench_r03*.json')) + glob.glob(os.path.join(ROOT, 'profiles', 'bench_r04*.json'))
    assert len(files) >= 10
    for fn in files:
        with open(fn) as fh:
            line = json.loads(fh.read().strip().splitlines()[-1])

        def walk(o, path=''):
            if isinstance(o, dict):
                for k, v in o.items():
                    if 'frac' in k and isinstance(v, (int, float)):
                        assert v <= 1.0, (fn, path + k, v)
                    walk(v, path + k + '.')
        walk(line)


def test_round4_bench_lines_carry_roofline_and_baseline_blocks():
    """the committed default lines of this round: `roofline` (dominant kernel, live HIP-event time, counter traffic of the very build),
    `eval_roofline` formed from counter bytes, `cpu_baseline` on the fp64 line, the energy pinned to the reference's"""
    for fn, need_cpu in (('bench_r04_final_256.json', True), ('bench_r04_final_256_f32.json', False)):
        with open(os.path.join(ROOT, 'profiles', fn)) as fh:
            d = json.loads(fh.read().strip().splitlines()[-1])
        r = d['roofline']
        assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and r['traffic']
        assert 0.9 < r['traffic'] / r['alg_bytes_per_launch'] < 1.1                 # nothing re-read
        assert 'rocprofv3' in d['eval_roofline']['hbm_bytes_basis'] and 0.5 < d['eval_roofline']['frac'] < 1.0
        assert d['reference_check']['ok'] and d['n_gpus'] == 1 and d['vs_baseline'] is None
        if need_cpu:
            assert d['cpu_baseline']['kind'] == 'port' and d['cpu_baseline']['cores'] >= 1 and d['cpu_baseline']['value'] > 0


def test_bench_workload_is_pinned_to_the_reference():
    with open(os.path.join(ROOT, 'tests', 'golden', 'bench_scalars.json')) as fh:
        ref = json.load(fh)
    assert 'cfg3_256' in ref and 'cfg3_128' in ref
    r = ref['cfg3_256']
    ok = bench.reference_check(256, 'cfg3', 'f64', r['E'] * (1 + 2e-12), r['mu'])
    bad = bench.reference_check(256, 'cfg3', 'f64', r['E'] * (1 + 2e-9), r['mu'])
    assert ok['ok'] and not bad['ok']
    assert bench.reference_check(96, 'cfg3', 'f64', 1.0, 1.0) is None         # no pin for that grid: reported as null
    # the pinned inputs are the bench's own: same recipe, same checksum
    import cases
    box, chi, vext, n_elec, _ = bench.make_inputs(128)
    assert abs(cases.checksum(chi[:8, :8, :8], vext[:8, :8, :8]) - ref['cfg3_128']['input_checksum']) < 1e-12
    assert n_elec == ref['cfg3_128']['n_elec']


def test_gradient_pin_of_the_bench_workload_accepts_the_reference_and_rejects_a_wrong_gradient():
    """round-4 verdict item 7: `reference_check` compares chi.grad of the timed call (L2 norm, sum, eight probes) with the
    reference's closure output; `grad_stats` forms the statistics from a tensor (whole grid, or one rank's x-slab)"""
    import torch
    with open(os.path.join(ROOT, 'tests', 'golden', 'bench_scalars.json')) as fh:
        r = json.load(fh)['cfg3_64']
    g = r['grad']
    ok = bench.reference_check(64, 'cfg3', 'f64', r['E'], r['mu'], dict(g))
    assert ok['ok'] and ok['grad_rel_dl2'] == 0.0 and ok['grad_probe_max_rel'] == 0.0
    for key, val in (('l2', g['l2'] * (1 + 1e-7)), ('sum', g['sum'] + 1e-6 * g['l2'] * 64 ** 1.5), ('probes', [p * (1 + 1e-6) for p in g['probes']])):
        bad = bench.reference_check(64, 'cfg3', 'f64', r['E'], r['mu'], dict(g, **{key: val}))
        assert not bad['ok'], key
    assert bench.reference_check(64, 'cfg3', 'f32', r['E'], r['mu'], dict(g, l2=g['l2'] * (1 + 1e-5)))['ok']        # fp32 bar: 5e-4
    # grad_stats: a whole grid and its two x-slabs give the same probes (each slab contributes the probes that fall into it)
    t = torch.arange(8 * 6 * 4, dtype=torch.double).reshape(8, 6, 4) * 0.01 - 0.5
    whole = bench.grad_stats(t)
    assert abs(whole['sum'] - float(t.sum())) < 1e-12 and abs(whole['l2'] - float((t * t).sum().sqrt())) < 1e-12
    assert whole['probes'] == [float(t.reshape(-1)[i]) for i in whole['probe_idx']]
    parts = [bench.grad_stats(t[:4], None, 0, t.numel()), bench.grad_stats(t[4:], None, 4, t.numel())]
    assert [a + b for a, b in zip(parts[0]['probes'], parts[1]['probes'])] == whole['probes']
    assert abs(parts[0]['sum'] + parts[1]['sum'] - whole['sum']) < 1e-12


def test_oracle_reproduces_the_bench_pin_at_64():
    """the CPU restatement (cpu_baseline leg) on the bench recipe equals the reference's closure energy"""
    import torch
    from oracle import refpath as rp
    with open(os.path.join(ROOT, 'tests', 'golden', 'bench_scalars.json')) as fh:
        ref = json.load(fh)['cfg3_64']
    box, chi, vext, n_elec, _ = bench.make_inputs(64)
    table = rp.term_table(torch.as_tensor(vext))
    fns = [table[k] for k in ('ion_electron', 'hartree', 'wgc99', 'pbe_x', 'pbe_c')]
    out = rp.closure(torch.as_tensor(box), torch.as_tensor(chi), n_elec, fns)
    E = float(out[0])
    assert abs(E - ref['E']) <= 1e-11 * abs(ref['E'])


def test_dump_outputs_writes_a_large_gradient_at_a_fixed_seeded_sample(tmp_path):
    """--dump-outputs: float files only, a gradient above the point budget at the same indices run after run, within 64 MB"""
    import torch
    E = {'ion_electron': -1.5, 'hartree': 0.25}
    g = torch.arange(160 ** 3, dtype=torch.double).reshape(160, 160, 160) * 1e-3
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), E, 0.125, g)
        runs.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
        assert sum(os.path.getsize(str(d / f)) for f in os.listdir(str(d))) < 64e6
    a, b = runs
    assert sorted(a) == ['energy_terms', 'grad', 'grad_index', 'mu']
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert list(a['energy_terms']) == [-1.5, 0.25] and list(a['mu']) == [0.125]
    idx = a['grad_index'].astype(np.int64)
    assert 0 < idx.size <= 1 << 21 and np.array_equal(a['grad'], g.reshape(-1).numpy()[idx])
    assert all(np.array_equal(a[f], b[f]) for f in a)


def test_source_stamp_is_stable_and_tracks_the_sources():
    a, b = bench.source_stamp(), bench.source_stamp()
    assert a == b and len(a) == 16


def test_multi_gpu_launch_refuses_without_enough_devices():
    """`python bench.py --gpus 2` on a box without two GPUs ends with a message and code 2 (no silent 1-GPU run)"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'OFDFT_BENCH_SHARE_GPU')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0'],
                       env=env, capture_output=True, text=True, timeout=300)
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('this box has two GPUs: the launch itself is covered by the -m gpu tier')
    assert p.returncode == 2 and '--gpus 2' in p.stderr, (p.returncode, p.stderr[-500:])


def test_host_cores_honours_override(monkeypatch):
    monkeypatch.setenv('OFDFT_CPU_THREADS', '3')
    assert bench.host_cores() == 3
    monkeypatch.delenv('OFDFT_CPU_THREADS')
    assert 1 <= bench.host_cores() <= (os.cpu_count() or 1)
