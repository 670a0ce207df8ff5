"""bench.py's multi-GPU launch is fail-closed: `--gpus N` either runs N ranks or exits non-zero -- it never prints a line
for fewer GPUs than asked (round-1 VERDICT: a bare `--gpus 8` ran on one GPU and printed "n_gpus": 1)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'NU_BENCH_DEVICE')}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_world_size_mismatch_is_refused():
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0'], {'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode == 2 and 'refusing' in r.stderr and '"metric"' not in r.stdout


def test_bare_multi_gpu_request_without_enough_devices_is_refused():
    # this container shows no GPU; a 1-GPU box shows one: either way `--gpus 2` must not fall back to one device
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("box has >= 2 GPUs: the bare launch would really run")
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0'], {})
    assert r.returncode == 2 and 'needs 2 visible GPUs' in r.stderr and '"metric"' not in r.stdout


def test_sum_rule_raises_when_gemm_time_exceeds_the_bracketed_step():
    """bench.py's consistency rule: launch times bracketed on the launch stream may not add up to more than the wall
    time of the step they were taken in."""
    import pytest
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    ok = bench.check_sum_rule("leg", 0.0400, 45.0)
    assert ok["ok"] and abs(ok["gemm_ms_in_bracketed_step"] - 40.0) < 1e-9
    with pytest.raises(bench.SumRuleError):
        bench.check_sum_rule("leg", 0.0460, 45.0)


def test_traffic_is_quoted_only_for_a_matching_profile():
    """roofline.traffic comes from a committed PMC pass only when that pass recorded this workload: same configuration, mean
    point counts within 5 %."""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    rec = json.load(open(os.path.join(bench.ROOT, 'profiles', 'r03', 'traffic_pmc.json')))['workload_record']
    pi, po = rec['mean_inner_points'], rec['mean_outer_points']
    nt, tn, src = bench.find_traffic_profile(rec['rays'], 1, rec['real_capture'], rec['mlp_dtype'], False, rec['bf16_storage'], pi * 1.03, po * 0.98)
    assert nt and tn and src.endswith('traffic_pmc.json')
    assert bench.find_traffic_profile(rec['rays'], 1, rec['real_capture'], rec['mlp_dtype'], False, rec['bf16_storage'], pi * 1.4, po) == (None, None, None)     # (no committed pass is that far out)
    assert bench.find_traffic_profile(rec['rays'], 2, rec['real_capture'], rec['mlp_dtype'], False, rec['bf16_storage'], pi, po) == (None, None, None)
    assert bench.find_traffic_profile(512, 1, rec['real_capture'], rec['mlp_dtype'], False, rec['bf16_storage'], pi, po) == (None, None, None)


def test_traffic_of_a_pass_with_batched_launches_is_rescaled_to_the_runs_launch_unit():
    """A counter pass counts KERNEL launches; outside the exact-fp32 mode bench.py times a level of the four light predictors as one
    launch.  A pass that recorded both counts (config 4: 80 kernels = 64 event launches per step) is matched on the run's own count
    and its bytes per kernel launch are rescaled to bytes per event launch; a run with another launch structure gets nothing."""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    d = json.load(open(os.path.join(bench.ROOT, 'profiles', 'r04', 'traffic_pmc_config4.json')))
    w = d['workload_record']
    assert w['nt_launches_per_step'] == 80.0 and w['nt_event_launches_per_step'] == 64.0
    nt, tn, src = bench.find_traffic_profile(w['rays'], 1, True, 'bf16', False, True, w['mean_inner_points'], w['mean_outer_points'], nt_launches=64)
    assert src.endswith('traffic_pmc_config4.json')
    assert abs(nt - d['gemm_nt_kernel']['hbm_bytes_per_launch'] * 80.0 / 64.0) < 1.0
    assert abs(tn - d['gemm_tn_kernel']['hbm_bytes_per_launch']) < 1.0                      # 34 kernels = 34 event launches
    assert bench.find_traffic_profile(w['rays'], 1, True, 'bf16', False, True, w['mean_inner_points'], w['mean_outer_points'],
                                      nt_launches=80) == (None, None, None)


def test_steps_below_one_is_refused():
    r = _run(['--steps', '0', '--warmup', '0'], {})
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr and '"metric"' not in r.stdout


def test_dump_outputs_writes_the_step_results_within_the_budget(tmp_path):
    """--dump-outputs: one float32 / float64 .npy per array a caller of the step holds; past the byte budget the large arrays are
    sampled at seeded indices, identically on every run."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    net = torch.nn.Linear(300, 200)
    net(torch.randn(5, 300)).sum().backward()
    out = {'ray_rgb': torch.rand(64, 3), 'acc': torch.rand(64, dtype=torch.float64), 'half': torch.rand(10, dtype=torch.bfloat16),
           'cand': torch.ones(64, dtype=torch.bool), '_paths': [torch.rand(3)], 'n': 3}
    arrays = bench.step_outputs(torch.tensor(0.5), {'loss_rgb': torch.rand(64)}, out, net)
    assert sorted(arrays) == ['grad.bias', 'grad.weight', 'log.loss_rgb', 'loss_total', 'out.acc', 'out.half', 'out.ray_rgb',
                              'param.bias', 'param.weight']

    rec = bench.dump_outputs(str(tmp_path / 'all'), arrays)
    assert rec['arrays'] == 9 and not rec['sampled']
    for k, v in arrays.items():
        a = np.load(tmp_path / 'all' / (k + '.npy'))
        assert a.dtype == (np.float64 if v.dtype == torch.float64 else np.float32) and a.shape == tuple(v.shape), k
        np.testing.assert_array_equal(a, v.detach().double().numpy())

    budget = 100_000                        # the 240 kB weight and its gradient must be cut to what the small arrays leave
    recs = [bench.dump_outputs(str(tmp_path / d), arrays, budget=budget) for d in ('a', 'b')]
    assert recs[0]['sampled'].keys() == {'param.weight', 'grad.weight'} and recs[0]['bytes'] <= budget
    assert recs[0]['sampled']['param.weight']['shape'] == [200, 300]
    for k in arrays:
        a, b = np.load(tmp_path / 'a' / (k + '.npy')), np.load(tmp_path / 'b' / (k + '.npy'))
        np.testing.assert_array_equal(a, b)
    w = np.load(tmp_path / 'a' / 'param.weight.npy')
    assert w.size == recs[0]['sampled']['param.weight']['elements'] and np.isin(w, net.weight.detach().numpy()).all()
