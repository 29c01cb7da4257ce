"""The launcher knobs of a context (sfe_tune / Context.tuning): checked names, checked values, restored on exit."""
import pytest

from sonar_slam_amd import _lib

pytestmark = pytest.mark.gpu


def test_tune_refuses_unknown_names_and_bad_values(ctx):
    for name, value in (("sw_wide", 1), ("SFE_SW_TIERS", 0), ("", 0),      # unknown (a deleted knob, the old env name)
                        ("sw_tiers", 2), ("sw_tiers", -1), ("sw_margin", 256), ("cfar_os_pref_x", 256),  # out of range
                        ("sw_multi_g", 17), ("sw_recm", 0), ("sw_reck", float("nan")),
                        ("sw_budget", 64.5), ("extract_capw", 0.25)):                 # a fraction for an integer knob
        with pytest.raises(_lib.SonarFEError, match="sfe_tune"):
            ctx.tune(name, value)
    assert ctx.tune("sw_tiers", 1) == 1 and ctx.tune("sw_margin", 15) == 15       # ... and nothing was changed


def test_tuning_restores_the_previous_values(ctx):
    assert ctx.tune("sw_reck", 3.0) == 3.0
    with ctx.tuning(sw_tiers=0, sw_reck=2.5, cfar_os_gated_min=0):
        assert ctx.tune("sw_tiers", 0) == 0 and ctx.tune("sw_reck", 2.5) == 2.5
        with pytest.raises(_lib.SonarFEError):
            with ctx.tuning(sw_tiny=0, sw_bogus=1):   # fails half way: what it set is put back
                pass
        assert ctx.tune("sw_tiny", 1) == 1
    assert ctx.tune("sw_tiers", 1) == 1 and ctx.tune("sw_reck", 3.0) == 3.0 and ctx.tune("cfar_os_gated_min", 40) == 40
    with pytest.raises(RuntimeError):
        with ctx.tuning(cost_many=0):
            raise RuntimeError("leaves the block")
    assert ctx.tune("cost_many", 1) == 1


def test_tuning_is_per_context(ctx):
    other = _lib.Context(ctx.device)
    try:
        with ctx.tuning(sw_multi=0):
            assert other.tune("sw_multi", 1) == 1
    finally:
        other.close()
