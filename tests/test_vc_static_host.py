"""CPU: the binding side of vc for trajectory converters from static features / device matrices / with the GV converter
(vcmi_vc_traj_static, vcmi_vc_traj_dev, vcmi_vc_trajgv, vcmi_vc_trajgv_dev) -- the Julia module reaches all four, the
reference's two-argument vc signatures are untouched, and the Python vc has the delta keyword."""
import inspect
import os
import re

import pytest

from conftest import ROOT

JL = os.path.join(ROOT, "voiceconversion.jl_amd", "julia", "VoiceConversionMI.jl")
NEW = ("vcmi_vc_traj_static", "vcmi_vc_traj_dev", "vcmi_vc_trajgv", "vcmi_vc_trajgv_dev")


@pytest.fixture(scope="module")
def vc():
    import __graft_entry__ as ge
    ge.build()
    import voiceconversion_jl_amd as m
    return m


def test_julia_module_calls_the_four_entries():
    text = open(JL).read()
    called = set(re.findall(r"ccall\(\(:([A-Za-z0-9_]+),\s*libvcmi\)", text))
    for sym in NEW:
        assert sym in called, f"the Julia module never calls {sym}"


def test_reference_vc_signatures_carry_no_keyword():
    text = open(JL).read()
    for needle in ("function vc(t::TrajectoryGMMMap, fm::Matrix{Float64})", "function vc(tgv::TrajectoryGVGMMMap, fm::Matrix{Float64})",
                   "function vc(g::GMMMap, fm::Matrix{Float64})"):
        assert needle in text, needle
    # the new capability sits on three-argument methods
    assert "function vc(t::TrajectoryGMMMap, fm::Matrix{Float64}, vs::Union{VarianceScaling,Nothing}; delta::Bool=false)" in text
    assert re.search(r"function vc\(tgv::TrajectoryGVGMMMap, fm::Matrix\{Float64\}, vs::Union\{VarianceScaling,Nothing\}; delta::Bool=false,\s*"
                     r"epochs::Int=100, α::Float64=1.0e-5\)", text)
    assert len(re.findall(r"function vc\(\w+::Trajectory(?:GV)?GMMMap, fm::DeviceMatrix, out::DeviceMatrix,[^\n]*\n[^\n]*stream::Ptr\{Cvoid\}=C_NULL\)",
                          text)) == 2


def test_python_vc_has_the_delta_keyword(vc):
    sig = inspect.signature(vc.vc)
    assert list(sig.parameters) == ["c", "fm", "postfilter", "delta"]
    assert sig.parameters["delta"].default is False and sig.parameters["postfilter"].default is None
    for cls in (vc.TrajectoryGMMMap, vc.TrajectoryGVGMMMap):
        p = inspect.signature(cls._vc).parameters
        assert p["delta"].default is False and p["postfilter"].default is None
    p = inspect.signature(vc.TrajectoryGVGMMMap._vc).parameters
    assert p["epochs"].default == 100 and p["alpha"].default == 1.0e-5
    from voiceconversion_jl_amd import _lib
    for sym in NEW:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
