#!/usr/bin/env python3
"""Record which launch policy nbody_create arrives at, case by case, on the device at hand.

    python tools/record_launch_policy.py --out tests/golden/launch_policy_parent.json

For every case a context is created and closed again: its launch_config(), sym_pool() and exchange_ranks() are recorded — or,
when the creation fails, the error's code and text.  No state is set and nothing is launched.  Public Python API only, so the
same file runs on any commit; tests/test_launch_policy.py replays the record against parallelnbody_amd.launch_policy on a CPU.

Every set of environment overrides (NBODY_SYM_*, NBODY_BLOCK_*) runs in a fresh child process, one after another: two of the
variables are latched at their first use.  The parent process never opens the device.

The file written: {"source", "device": {"compute_units", "total_bytes"}, "fields": [keyword names], "expect_fields": [result keys],
"records": [{"env", "expect", "cases"}, ...]}: one record per distinct outcome under one set of overrides — "expect" holds the
recorded values in the order of "expect_fields", or {"code", "error"}; "cases" the keyword values (in the order of "fields") of
every case that arrived at it.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# both sides of every size threshold of the policy
SIZES = (1, 2, 255, 2000, 4096, 6655, 6656, 9215, 9216, 12287, 12288, 16384, 16385, 17407, 17408, 20479, 20480, 22527, 22528,
         24575, 24576, 40959, 40960, 49152, 65536, 90111, 90112, 100003, 131071, 131072, 139263, 139264)
PRECISIONS = ("f32", "f32_kahan", "f64")
ALGORITHMS = (0, 1, 2)     # auto, tiled, symmetric
ZERO_MODES = (0, 1, 2)     # exact, select, floor


FIELDS = ("n_total", "precision", "algorithm", "zero_mode", "eps", "i_begin", "i_count", "tile", "i_per_thread", "j_split")
EXPECT_FIELDS = ("tile", "i_per_thread", "j_split", "blocks", "threads", "algorithm", "super_tile", "kernel", "plan", "pool_bytes", "phases",
                 "exchange_ranks")
DEFAULTS = dict(i_begin=0, i_count=0, precision="f32", eps=0.0, tile=0, i_per_thread=0, j_split=0, zero_mode=0, algorithm=0)


def write_record(path, source, device, cases):
    """cases: [{"env", "kw", "expect"}, ...] -> the file, cases with one outcome on one line."""
    records = {}
    for c in cases:
        key = (json.dumps(c["env"], sort_keys=True), json.dumps(c["expect"], sort_keys=True))
        expect = c["expect"] if "code" in c["expect"] else [c["expect"][f] for f in EXPECT_FIELDS]
        rec = records.setdefault(key, {"env": c["env"], "expect": expect, "cases": []})
        row = [c["kw"].get(f, DEFAULTS.get(f)) for f in FIELDS]
        while len(row) > 1 and row[-1] == DEFAULTS[FIELDS[len(row) - 1]]:
            row.pop()                                             # trailing defaults are left out
        rec["cases"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write('{"source": %s,\n "device": %s,\n "fields": %s,\n "expect_fields": %s,\n "records": [\n' %
                (json.dumps(source), json.dumps(device), json.dumps(FIELDS), json.dumps(EXPECT_FIELDS)))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in records.values()))
        f.write("\n]}\n")


def kw(n_total, **more):
    """The keywords of a case without the ones left at their defaults."""
    assert set(more) <= set(DEFAULTS), more
    return dict(n_total=n_total, **{k: v for k, v in more.items() if v != DEFAULTS[k]})


def case_groups():
    """[(env, [kw, ...]), ...]: one child process per group."""
    base = []
    for n, prec, algo, zm, eps in itertools.product(SIZES, PRECISIONS, ALGORITHMS, ZERO_MODES, (0.0, 0.5)):
        base.append(kw(n, precision=prec, algorithm=algo, zero_mode=zm, eps=eps))
    for n, prec, zm, eps in itertools.product((262144, 1 << 20), PRECISIONS, ZERO_MODES, (0.0, 0.5)):
        base.append(kw(n, precision=prec, zero_mode=zm, eps=eps))
    # sharded slices
    slices = [(65536, r, k) for r in (2, 4, 8) for k in range(r)] + [(49152, 3, k) for k in range(3)]
    slices += [(n, 8, k) for n in (131072, 1 << 20) for k in (0, 7)]
    for (n, ranks, k), prec, algo in itertools.product(slices, PRECISIONS, (0, 2)):
        base.append(kw(n, i_begin=k * (n // ranks), i_count=n // ranks, precision=prec, algorithm=algo))
    for prec, algo in itertools.product(PRECISIONS, ALGORITHMS):
        base.append(kw(65536, i_begin=100, i_count=300, precision=prec, algorithm=algo))
    # forced geometries, the refused combinations among them
    forced = [dict(i_per_thread=v) for v in (1, 2, 4, 8, 16)] + [dict(tile=v) for v in (64, 512)] + [dict(j_split=v) for v in (1, 8)]
    forced += [dict(tile=128, i_per_thread=2, j_split=4), dict(tile=100), dict(i_per_thread=3), dict(j_split=-1)]
    for n, prec, algo, f in itertools.product((20000, 65536), PRECISIONS, ALGORITHMS, forced):
        base.append(kw(n, precision=prec, algorithm=algo, **f))
    for n, ranks, ipt in ((65536, 4, 16), (65536, 8, 8), (65536, 16, 16), (49152, 3, 16)):   # slices and whole i-sets
        base.append(kw(n, i_begin=0, i_count=n // ranks, i_per_thread=ipt))
        base.append(kw(n, i_begin=0, i_count=n // ranks, i_per_thread=ipt, algorithm=2))
    # arguments nbody_create refuses
    base += [kw(0), kw(-5), kw(1000, i_begin=1000), kw(1000, i_begin=-1), kw(1000, i_begin=500, i_count=501), kw(1000, zero_mode=3),
             kw(1000, algorithm=3), kw(1000, eps=-1.0)]
    groups = [({}, base)]
    for even in ("0", "1"):
        groups.append(({"NBODY_SYM_EVEN": even},
                       [kw(n, precision=prec, algorithm=algo) for n, prec, algo in itertools.product((12288, 20480, 65536), PRECISIONS, (0, 2))]))
    groups.append(({"NBODY_SYM_POOL_BUDGET_MB": "2"},
                   [kw(65536, precision=prec) for prec in PRECISIONS] +
                   [kw(65536, precision=prec, i_begin=k * 16384, i_count=16384) for prec in ("f32", "f32_kahan") for k in range(4)]))
    groups.append(({"NBODY_SYM_IPT": "8"}, [kw(65536, precision=prec, algorithm=algo) for prec, algo in itertools.product(PRECISIONS, (0, 2))]))
    groups.append(({"NBODY_BLOCK_MAX_N": "1"}, [kw(2000, precision=prec, algorithm=algo) for prec, algo in itertools.product(PRECISIONS, ALGORITHMS)]))
    return groups


def record_one(nb, kwargs):
    # The text of a refused creation stays what nbody_last_error(NULL) reports until a creation succeeds, and a later refusal may
    # quote it: every case starts after a small creation that succeeded, so that no record depends on the cases before it.
    nb.NBodyEngine(2).close()
    try:
        with nb.NBodyEngine(**kwargs) as e:
            out = e.launch_config()
            out["pool_bytes"], out["phases"] = e.sym_pool()
            out["exchange_ranks"] = e.exchange_ranks()
            return out
    except nb.NBodyError as err:
        text = str(err)
        prefix = f"nbody error {err.code}: "
        return {"code": err.code, "error": text[len(prefix):] if text.startswith(prefix) else text}


def child(group, path):
    import torch
    import parallelnbody_amd as nb
    env, cases = case_groups()[group]
    props = torch.cuda.get_device_properties(0)
    device = {"name": props.name, "compute_units": int(props.multi_processor_count), "total_bytes": int(torch.cuda.mem_get_info(0)[1])}
    records = [{"env": env, "kw": k, "expect": record_one(nb, k)} for k in cases]
    with open(path, "w") as f:
        json.dump({"device": device, "cases": records}, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_policy_parent.json"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.child_out)
    device, cases = None, []
    clean = {k: v for k, v in os.environ.items() if not k.startswith("NBODY_")}
    with tempfile.TemporaryDirectory() as tmp:
        for g, (env, group_cases) in enumerate(case_groups()):
            path = os.path.join(tmp, f"group{g}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(g), "--child-out", path],
                           env={**clean, **env}, check=True, timeout=900)
            with open(path) as f:
                got = json.load(f)
            assert device in (None, got["device"]) and len(got["cases"]) == len(group_cases)
            device = got["device"]
            cases += got["cases"]
            print(f"group {g} {env}: {len(group_cases)} cases", flush=True)
    write_record(a.out, "contexts created and closed on the device (tools/record_launch_policy.py)", device, cases)
    failed = sum(1 for c in cases if "code" in c["expect"])
    print(f"{len(cases)} cases ({failed} refused creations) on {device} -> {a.out}")


if __name__ == "__main__":
    main()
