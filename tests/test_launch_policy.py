"""The launch policy (csrc/launch_policy.cpp) on the CPU: which kernel, geometry and plan a context gets is a function of its
parameters, the device's CU count and its total memory, and parallelnbody_amd.launch_policy evaluates that function without a device.

tests/golden/launch_policy_parent.json is what the library decided, case by case, before the policy became a unit of its own: the
cases of tools/record_launch_policy.py (both sides of every size threshold, every precision, algorithm and zero mode, sharded
slices, forced geometries, refused creations, environment overrides) for an MI355X's CU count and memory; its "source" field says
how the committed record was made.  The policy must reproduce it key for key; a threshold that moves shows up here, on a CPU,
and not as a speed change on a GPU.  Re-record (that tool, on a device) only when a threshold is moved on purpose."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_policy_parent.json")
GIB = 1 << 30


def _groups():
    """The record's cases grouped by their environment overrides: (device, [(env, [{"kw", "expect"}, ...]), ...])."""
    with open(GOLDEN) as f:
        rec = json.load(f)
    groups = []
    for r in rec["records"]:
        if not groups or groups[-1][0] != r["env"]:
            groups.append((r["env"], []))
        expect = r["expect"] if isinstance(r["expect"], dict) else dict(zip(rec["expect_fields"], r["expect"]))
        groups[-1][1].extend({"kw": dict(zip(rec["fields"], row)), "expect": expect} for row in r["cases"])
    return rec["device"], groups


def _replay(nb, device, cases):
    """Mismatches of launch_policy against the recorded cases: [(kw, key, recorded, got), ...]."""
    bad = []
    for case in cases:
        kw, want = case["kw"], case["expect"]
        try:
            got = nb.launch_policy(compute_units=device["compute_units"], device_total_bytes=device["total_bytes"], **kw)
        except nb.NBodyError as err:
            text = str(err)
            got = {"code": err.code, "error": text[len(f"nbody error {err.code}: "):]}
        for key in want:
            if key not in got or got[key] != want[key]:
                bad.append((kw, key, want[key], got.get(key, "<missing>")))
    return bad


def _child(group):
    sys.path.insert(0, ROOT)
    import parallelnbody_amd as nb
    device, groups = _groups()
    env, cases = groups[group]
    assert all(os.environ.get(k) == v for k, v in env.items())
    print(json.dumps(_replay(nb, device, cases)))


N_GROUPS = len(_groups()[1])


def test_the_record_covers_what_it_should():
    device, groups = _groups()
    assert device["compute_units"] > 0 and device["total_bytes"] > 100 * GIB
    assert groups[0][0] == {} and len(groups[0][1]) > 2000
    envs = [env for env, _ in groups[1:]]
    assert {"NBODY_SYM_EVEN": "0"} in envs and {"NBODY_SYM_EVEN": "1"} in envs and {"NBODY_SYM_POOL_BUDGET_MB": "2"} in envs
    assert {"NBODY_SYM_IPT": "8"} in envs and {"NBODY_BLOCK_MAX_N": "1"} in envs
    refused = [c for _, cases in groups for c in cases if "code" in c["expect"]]
    assert len(refused) > 100 and {c["expect"]["code"] for c in refused} == {-1, -6}      # NBODY_ERR_INVALID, NBODY_ERR_UNSUPPORTED
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize("group", range(N_GROUPS))
def test_policy_reproduces_the_record(nb, group):
    # every group in a fresh child process: NBODY_* scrubbed but for the group's own overrides, and two of the variables are
    # latched at their first use
    env = {k: v for k, v in os.environ.items() if not k.startswith("NBODY_")}
    env.update(_groups()[1][group][0])
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(group)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    bad = json.loads(out.stdout.strip().splitlines()[-1])
    assert not bad, f"{len(bad)} differences from the record, the first ones: {bad[:5]}"


@pytest.fixture
def policy(nb, monkeypatch):
    for k in [k for k in os.environ if k.startswith("NBODY_")]:
        monkeypatch.delenv(k)
    return nb.launch_policy


@pytest.mark.parametrize("n", [131072, 1 << 20])
def test_the_ranks_of_a_sharded_job_get_equal_policies(policy, n):
    # sharded bit-parity rests on it.  Every decision is equal — kernel, geometry, bodies per lane, slots, K, shortest strip, phases,
    # detector —; what may differ is the size of the rank's own plan: `blocks` (its work items: the ranks' strip counts differ by a
    # few, as tests/test_rank_geometries_gpu.py allows) and with it `pool_bytes` (one segment or two per work item)
    ranks = []
    for r in range(8):
        for prec in ("f32", "f32_kahan", "f64"):
            cfg = policy(n, i_begin=r * (n // 8), i_count=n // 8, precision=prec)
            cfg.pop("blocks")
            cfg.pop("pool_bytes")
            ranks.append((r, prec, cfg))
    for r, prec, cfg in ranks:
        assert cfg == next(c for r0, p0, c in ranks if r0 == 0 and p0 == prec), (r, prec)
        assert cfg["algorithm"] == "symmetric" and cfg["exchange_ranks"] == 8


def test_n_2p23_runs_the_symmetric_pass_in_phases_on_a_288_gib_card(policy):
    # what tests/test_parity_gpu.py::test_auto_stays_symmetric_at_n_2p23 observes on the device (tens of GB, 7e13 interactions)
    cfg = policy(1 << 23, device_total_bytes=288 * GIB)
    assert cfg["algorithm"] == "symmetric" and cfg["i_per_thread"] == 16 and cfg["plan"] == "guided"
    assert cfg["phases"] >= 4 and cfg["pool_bytes"] <= 32 * GIB


def test_n_2p22_stays_one_pass_on_a_288_gib_card(policy):
    cfg = policy(1 << 22, device_total_bytes=288 * GIB)
    assert cfg["algorithm"] == "symmetric" and cfg["phases"] == 1


def test_fp64_at_n_2p23_leaves_to_the_one_sided_kernel(policy):
    cfg = policy(1 << 23, device_total_bytes=288 * GIB, precision="f64")
    assert cfg["algorithm"] == "tiled" and cfg["kernel"] == "forces_tile_kernel" and cfg["pool_bytes"] == 0


@pytest.mark.parametrize("n,kw", [(2000, {}), (4096, {"precision": "f64"}), (6000, {"precision": "f32_kahan"}), (16384, {}), (20480, {}),
                                  (65536, {}), (65536, {"precision": "f64"}), (65536, {"i_begin": 16384, "i_count": 16384})])
def test_an_unknown_cu_count_means_256(policy, n, kw):
    want = policy(n, compute_units=256, **kw)
    assert policy(n, compute_units=0, **kw) == want and policy(n, compute_units=-3, **kw) == want
    if want["algorithm"] == "symmetric":                                # (the count does matter: resident workgroups)
        assert policy(n, compute_units=304, **kw)["sym_slots"] * 256 == want["sym_slots"] * 304


def test_without_the_cards_size_no_plan_is_refused_for_its_size(nb, policy):
    # 2^22: a one-pass pool of 35 GiB — beyond a third of a 64 GiB card, where the pass runs in phases; fp64 has no phased form
    assert policy(1 << 22, device_total_bytes=64 * GIB)["phases"] > 1
    assert policy(1 << 22, device_total_bytes=0)["phases"] == 1
    assert policy(1 << 20, device_total_bytes=16 * GIB, precision="f64")["algorithm"] == "tiled"
    with pytest.raises(nb.NBodyError, match="a third of the device memory"):
        policy(1 << 20, device_total_bytes=16 * GIB, precision="f64", algorithm=2)
    assert policy(1 << 20, device_total_bytes=0, precision="f64", algorithm=2)["algorithm"] == "symmetric"


def test_describe_reports_like_a_refused_creation(nb, policy):
    with pytest.raises(nb.NBodyError) as e:
        policy(1000, tile=100)
    assert e.value.code == nb._lib.ERR_INVALID and "tile must be 64, 128, 256 or 512" in str(e.value)
    with pytest.raises(nb.NBodyError) as e:
        policy(20000, i_per_thread=16, precision="f64")
    assert e.value.code == nb._lib.ERR_UNSUPPORTED and "plain fp32 symmetric kernel only" in str(e.value)
    policy(2000)
    assert nb.lib().nbody_last_error(None) == b""          # as after a creation that succeeded


if __name__ == "__main__":
    _child(int(sys.argv[1]))
