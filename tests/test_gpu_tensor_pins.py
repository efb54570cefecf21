"""GPU: the bytes of every tensor-pull family, pinned.  The other pull tests hold the kernels to float64 models within a bound; a
change that promises the same output to the last bit is held to tests/golden/tensor_pull_pins.json instead: the SHA-256 of each
case's output tensor, recorded from the build before the change by tests/golden/make_tensor_pull_pins.py, which also holds the list
of cases (all 30 instantiations of each family; the shapes are described there)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_tensor_pull_pins", os.path.join(_GOLDEN, "make_tensor_pull_pins.py"))
pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins)


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(scope="module")
def runner(built):
    run = pins.Runner(built)
    yield run
    run.close()


@pytest.fixture(scope="module")
def want():
    return json.load(open(pins.PINS))


def test_the_pin_file_covers_the_case_list(want):
    cases = pins.cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    for family in pins.FAMILIES:
        mine = [c for c in cases if c[1] == family]
        assert len(mine) % 30 == 0 and len({c[4:] for c in mine}) == 30, family


def _check_family(built, runner, want, family):
    cases = [c for c in pins.cases() if c[1] == family]
    differing = [c[0] for c in cases if runner.run(c) != want[c[0]]]
    assert built.device_errors() == 0
    assert not differing, (family, len(differing), "of", len(cases), differing[:8])


def test_whole_picture_pull_reproduces_its_pins(built, runner, want):
    _check_family(built, runner, want, "out")


def test_bilinear_stretch_resize_reproduces_its_pins(built, runner, want):
    _check_family(built, runner, want, "resize")


def test_antialiased_and_letterboxed_resize_reproduces_its_pins(built, runner, want):
    _check_family(built, runner, want, "aa")


def test_region_pull_reproduces_its_pins(built, runner, want):
    _check_family(built, runner, want, "roi")


def test_remap_pull_reproduces_its_pins(built, runner, want):
    _check_family(built, runner, want, "remap")
