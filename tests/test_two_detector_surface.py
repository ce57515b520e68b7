"""CPU-only checks of the two-detector pipeline's surface: `full_pipeline_two_detectors` takes the aux detector names (`full_pipeline`
keeps the reference's signature, test_cabi.py), refuses unknown ones before it touches a GPU, and the binding knows `ttup_vitpose_forward_frames` (test_cabi.py checks that the library exports it)."""
import inspect

import pytest

import hubconf
from upliftingtabletennis_amd import _lib


def test_hub_takes_the_aux_detectors():
    params = inspect.signature(hubconf.full_pipeline_two_detectors).parameters
    assert params['ball_aux'].default == 'vitpose' and params['table_aux'].default == 'vitpose'
    assert list(inspect.signature(hubconf.full_pipeline).parameters) == []
    from upliftingtabletennis_amd.interface import TableTennisPipeline
    params = inspect.signature(TableTennisPipeline).parameters
    assert params['ball_aux'].default is None and params['table_aux'].default is None


@pytest.mark.parametrize('kw,exc', [({'ball_aux': 'hrnet'}, ValueError), ({'table_aux': 'wasb'}, ValueError), ({'ball_aux': 1}, ValueError),
                                    ({'ball_aux': 'segformerpp_b2'}, NotImplementedError),
                                    ({'table_aux': 'segformerpp_b5'}, NotImplementedError)])
def test_unknown_aux_names_are_refused_first(kw, exc):
    with pytest.raises(exc):
        hubconf.full_pipeline_two_detectors(**kw)


def test_binding_declares_forward_frames():
    ret, args = _lib.SIGNATURES['ttup_vitpose_forward_frames']
    assert len(args) == 9
