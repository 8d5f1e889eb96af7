"""merge_vcfs in bounded memory, the host side: the plan of the library (snpgpu_merge_plan: no device, no context) and the option
that carries a budget to it (--mergeDeviceBytes / SNPGPU_MERGE_DEVICE_BYTES)."""
import pytest

GIB = 1 << 30
MAX_RECORDS = (1 << 31) - 2
# BASELINE configs[4]: 10 000 samples x 200 000 sites, 2 * 10^9 records of about 80 bytes
BIG = dict(n_files=10000, n_sites=200000, total_input_bytes=160 * 10 ** 9)


def _plan(**kw):
    from snp_pipeline_amd.device import Device
    return Device.merge_plan(**kw)


@pytest.fixture
def env(tmp_path, monkeypatch):
    monkeypatch.setenv("errorOutputFile", str(tmp_path / "error.log"))
    monkeypatch.delenv("SNPGPU_MERGE_DEVICE_BYTES", raising=False)
    return tmp_path


def test_option_and_environment(env, monkeypatch):
    from snp_pipeline_amd import cfsan_snp_pipeline as cli
    from snp_pipeline_amd import merge_vcfs as mv
    assert not hasattr(cli.parse_command_line("merge_vcfs dirs.txt"), "mergeDeviceBytes")       # (additive: the namespace of the reference otherwise)
    assert cli.parse_command_line("merge_vcfs --mergeDeviceBytes 123456 dirs.txt").mergeDeviceBytes == "123456"
    assert cli.parse_command_line("hot_path_batch --mergeVcfs --mergeDeviceBytes 77 dirs.txt ref.fasta").mergeDeviceBytes == "77"
    assert mv.merge_device_bytes(None) == 0                      # the default
    assert mv.merge_device_bytes("123456") == 123456 and mv.merge_device_bytes(0) == 0
    monkeypatch.setenv("SNPGPU_MERGE_DEVICE_BYTES", "4096")
    assert mv.merge_device_bytes(None) == 4096 and mv.merge_device_bytes("5") == 5               # the option goes before the environment
    for bad in ("-1", "1.5", "12k", "", " "):
        with pytest.raises(SystemExit):
            mv.merge_device_bytes(bad)
        text = open(str(env / "error.log")).read()
        assert "--mergeDeviceBytes / SNPGPU_MERGE_DEVICE_BYTES must be a non-negative integer" in text
    monkeypatch.setenv("SNPGPU_MERGE_DEVICE_BYTES", "lots")
    with pytest.raises(SystemExit):
        mv.merge_device_bytes(None)


def test_the_budget_reaches_the_device_object_only_when_set(env, tmp_path, monkeypatch):
    from snp_pipeline_amd import merge_vcfs as mv
    calls = []

    class Plain(object):                                         # a device object of before the option: no such parameter
        def merge_vcf_files(self, paths, out_path, own_lines=b""):
            calls.append(("plain", None))
            return {}

    class Budgeted(object):
        def merge_vcf_files(self, paths, out_path, own_lines=b"", device_bytes=0):
            calls.append(("budgeted", device_bytes))
            return {}

    mv.merge_files_device(Plain(), ["a"], "out")
    mv.merge_files_device(Budgeted(), ["a"], "out")
    mv.merge_files_device(Budgeted(), ["a"], "out", device_bytes=4096)
    assert calls == [("plain", None), ("budgeted", 0), ("budgeted", 4096)]


def test_plan_of_the_largest_named_workload():
    """Today's call refuses these figures before it reads a byte (2.9 * 10^9 records by its bound, over 2^31 - 2); under 200 GiB
    the plan is a handful of site rounds."""
    plan = _plan(device_bytes=200 * GIB, **BIG)
    print(plan)
    assert 2 <= plan["site_rounds"] <= 8 and plan["input_passes"] == 1 + plan["site_rounds"]
    assert plan["sites_per_round"] * BIG["n_files"] <= MAX_RECORDS
    assert plan["sites_per_round"] * plan["site_rounds"] >= BIG["n_sites"]
    assert plan["sites_per_round"] * (plan["site_rounds"] - 1) < BIG["n_sites"]                  # (no round of nothing)
    # nothing has wrapped: the plan holds at least the slots of a round (164 bytes each) and no more than the budget
    assert plan["sites_per_round"] * BIG["n_files"] * 164 < plan["device_bytes"] <= 200 * GIB
    assert plan["device_bytes"] > 150 * GIB                      # the budget is used, not a sliver of it
    # more than 2^31 - 2 records can never be held whole: without a budget it is one round of all sites after the key pass ...
    free = _plan(device_bytes=0, **BIG)
    assert free["input_passes"] == 2 and free["site_rounds"] == 1 and BIG["n_sites"] <= free["sites_per_round"] <= MAX_RECORDS // BIG["n_files"]
    # ... and a merge the single pass does hold is the single pass
    small = dict(n_files=1000, n_sites=50000, total_input_bytes=4 * 10 ** 9)
    whole = _plan(device_bytes=0, **small)
    assert whole["input_passes"] == 1 and whole["site_rounds"] == 0 and whole["sites_per_round"] >= small["n_sites"]
    assert 11 * 10 ** 9 < whole["device_bytes"] < 40 * 10 ** 9   # (the issue's "about 13 GB" of records, and the key, sort and table arrays)
    exact = _plan(device_bytes=whole["device_bytes"], **small)
    assert exact["input_passes"] == 1 and exact["device_bytes"] == whole["device_bytes"] and exact["sites_per_round"] >= small["n_sites"]
    under = _plan(device_bytes=whole["device_bytes"] - 1, **small)
    assert under["input_passes"] == 1 + under["site_rounds"] > 1 and under["sites_per_round"] == small["n_sites"] - 1


def test_plan_is_monotone_in_the_budget():
    from snp_pipeline_amd.device import SnpGpuError
    for figures in (BIG, dict(n_files=130, n_sites=41, total_input_bytes=520000), dict(n_files=4, n_sites=160, total_input_bytes=60000),
                    dict(n_files=300, n_sites=5 * 10 ** 6, total_input_bytes=300 * 400 * 10 ** 6)):
        last = None
        budgets = sorted(set([1, 1 << 20] + [int((48 << 20) * 1.07 ** k) for k in range(140)]))
        for budget in budgets:
            try:
                plan = _plan(device_bytes=budget, **figures)
            except SnpGpuError as err:
                assert err.code == -3 and last is None, (budget, figures)       # refused below a threshold only, never above a plan
                continue
            assert plan["device_bytes"] <= budget
            if last is not None:
                assert plan["sites_per_round"] >= last["sites_per_round"] and plan["input_passes"] <= last["input_passes"], (budget, plan, last)
            last = plan
        assert last is not None
        print(figures, last)


def test_a_budget_below_one_site_is_refused_with_the_bytes_needed():
    from snp_pipeline_amd.device import SnpGpuError
    figures = dict(n_files=130, n_sites=41, total_input_bytes=520000)
    with pytest.raises(SnpGpuError) as err:
        _plan(device_bytes=1 << 20, **figures)
    assert err.value.code == -3
    import re
    needed = int(re.search(r"needs (\d+) bytes", str(err.value)).group(1))
    assert needed > 1 << 20
    assert _plan(device_bytes=needed, **figures)["sites_per_round"] >= 1          # what it names is enough ...
    with pytest.raises(SnpGpuError):
        _plan(device_bytes=needed - 1, **figures)                                  # ... and nothing less is
