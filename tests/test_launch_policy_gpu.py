"""A created context reports what parallelnbody_amd.launch_policy says for the live device: nbody_create carries out the policy of
csrc/launch_policy.cpp and nothing else.  One case per branch; contexts are created and closed only, no kernel runs.

The device's facts come from torch here and from the HIP runtime inside nbody_create; the two may word the card's total memory a
little differently.  That cannot matter at these sizes: the only use of it is the "pool beyond a third of the card" test, and the
largest pool below is a few hundred MB."""
import pytest

pytestmark = pytest.mark.gpu

CASES = [
    dict(n_total=2000),                                                      # block kernel, plain fp32
    dict(n_total=4096, precision="f32_kahan"),                               # block kernel, bodies per workgroup
    dict(n_total=9000, precision="f64"),                                     # tile kernel
    dict(n_total=20000, zero_mode=1),                                        # compare+select: one-sided tile kernel
    dict(n_total=16384, algorithm=2),                                        # guided strips
    dict(n_total=65536, algorithm=1),                                        # packed tile kernel with its detector
    dict(n_total=20480),                                                     # even shares, eight bodies per lane
    dict(n_total=100003),                                                    # even shares, two items per slot, ragged
    dict(n_total=139264),                                                    # past the even shares: guided
    dict(n_total=32768, precision="f32_kahan"),                              # Kahan, even shares
    dict(n_total=65536, precision="f32_kahan", eps=0.5),                     # Kahan, guided
    dict(n_total=65536, precision="f64"),                                    # fp64 symmetric
    dict(n_total=65536, i_begin=16384, i_count=16384),                       # sharded slice
    dict(n_total=49152, i_begin=32768, i_count=16384, precision="f64"),      # sharded fp64 slice
    dict(n_total=65536, i_per_thread=8, zero_mode=2),                        # forced bodies per lane, eps floor
    dict(n_total=65536, i_begin=100, i_count=300, algorithm=2),              # refused: no plan for this slice
    dict(n_total=20000, i_per_thread=16, precision="f64"),                   # refused: no such kernel
]


def _facts():
    import torch
    props = torch.cuda.get_device_properties(0)
    return dict(compute_units=int(props.multi_processor_count), device_total_bytes=int(torch.cuda.mem_get_info(0)[1]))


def _created(nb, kw):
    try:
        with nb.NBodyEngine(**kw) as e:
            got = e.launch_config()
            got["pool_bytes"], got["phases"] = e.sym_pool()
            got["exchange_ranks"] = e.exchange_ranks()
            return got
    except nb.NBodyError as err:
        return {"code": err.code, "error": str(err)}


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_a_created_context_reports_the_policy(nb, monkeypatch, kw):
    import os
    for var in [v for v in os.environ if v.startswith("NBODY_")]:
        monkeypatch.delenv(var)
    try:
        want = nb.launch_policy(**kw, **_facts())
    except nb.NBodyError as err:
        want = {"code": err.code, "error": str(err)}
    got = _created(nb, kw)
    assert ("code" in got) == ("code" in want), (got, want)
    assert got == {k: want[k] for k in got}


def test_forced_pool_phases(nb, monkeypatch):
    # NBODY_SYM_POOL_BUDGET_MB is read when a context is created, so it can be set here
    monkeypatch.setenv("NBODY_SYM_POOL_BUDGET_MB", "2")
    kw = dict(n_total=65536)
    want = nb.launch_policy(**kw, **_facts())
    got = _created(nb, kw)
    assert got["phases"] > 1 and got["plan"] == "guided"
    assert got == {k: want[k] for k in got}
