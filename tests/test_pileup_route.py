"""hot_path_batch --pileupRoute / $SNPGPU_PILEUP_ROUTE: the option, the variable, and what ``auto`` decides (no device needed)."""
import pytest

from snp_pipeline_amd import cfsan_snp_pipeline as cli
from snp_pipeline_amd import hot_path


def _parse(*more):
    return cli.parse_argument_list(["hot_path_batch", "dirs.txt", "ref.fasta"] + list(more))


def test_the_option_is_parsed_and_defaults_to_the_environment_then_auto(monkeypatch, tmp_path):
    monkeypatch.delenv("SNPGPU_PILEUP_ROUTE", raising=False)
    assert _parse().pileupRoute is None and hot_path.pileup_route_setting(_parse().pileupRoute) == "auto"
    for route in hot_path.PILEUP_ROUTES:
        assert hot_path.pileup_route_setting(_parse("--pileupRoute", route).pileupRoute) == route
    with pytest.raises(SystemExit):
        _parse("--pileupRoute", "twice")
    monkeypatch.setenv("SNPGPU_PILEUP_ROUTE", "Stream")
    assert hot_path.pileup_route_setting(None) == "stream"
    assert hot_path.pileup_route_setting("resident") == "resident"          # the option goes before the variable
    monkeypatch.setenv("SNPGPU_PILEUP_ROUTE", "sideways")
    monkeypatch.setenv("errorOutputFile", str(tmp_path / "error.log"))
    with pytest.raises(SystemExit) as ei:
        hot_path.pileup_route_setting(None)
    assert ei.value.code == 100


@pytest.mark.parametrize("mode, rank_bytes, budget, want", [
    ("existing", 1001, 1000, "stream"), ("varscan", 1001, 1000, "stream"),
    ("existing", 1000, 1000, "resident"), ("varscan", 0, 0, "resident"), ("existing", 1, 0, "stream"),
    ("device", 1001, 1000, "resident"), ("device", 10 ** 13, 1, "resident"),        # two crossings past the budget are inherent there
    ("existing", 540 * 10 ** 9, 264 * 10 ** 9, "stream"),
])
def test_auto_is_a_function_of_mode_rank_bytes_and_budget(mode, rank_bytes, budget, want):
    assert hot_path.resolve_pileup_route("auto", mode, rank_bytes, budget) == want


def test_an_explicit_route_is_kept_whatever_the_sizes():
    for mode in ("existing", "varscan", "device"):
        assert hot_path.resolve_pileup_route("resident", mode, 10 ** 12, 1) == "resident"
    for mode in hot_path.STREAM_MODES:
        assert hot_path.resolve_pileup_route("stream", mode, 1, 10 ** 12) == "stream"
