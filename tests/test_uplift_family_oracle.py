"""CPU side of the uplift model family (every variant the reference's get_model builds): schemas, seeded weights, blobs,
argument errors and the by-path checkpoint loader's variant choice, against tests/golden/uplift_family_schema.json (the
reference's own state_dict() key lists, tools/make_goldens_uplift_family.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

from upliftingtabletennis_amd import arch, inference, uplift, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# sha256 of pack_uplift_blob(random_uplift_state_dict(3, size), size) at the commit before the variants existed
PARENT_BLOB_SHA256 = {'small': 'd82a0ad8874471e4d2420a05fd70742f2660a5cfbda3c9cb364c4e51ff47f6b6',
                      'large': 'c1dee3fbb13bb06c99d6ed303c932ae197d570a067a75256f48a0c491d4c0c98'}


def _schema():
    with open(os.path.join(GOLDEN, 'uplift_family_schema.json')) as f:
        return json.load(f)


def test_there_are_eighteen_variants():
    v = arch.uplift_variants()
    assert len(v) == len(set(v)) == 18
    stored = _schema()
    for name, mode, _ in v:
        assert '%s/small/%s' % (name, mode) in stored
    assert {k.split('/')[1] for k in stored} == set(arch.UPLIFT_SIZES)


@pytest.mark.parametrize('key', sorted(_schema()))
def test_schema_and_seeded_weights_follow_the_reference(key):
    name, size, mode = key.split('/')
    ref = [(k, tuple(s)) for k, s in _schema()[key]]
    assert arch.uplift_variant_schema(name, size, mode) == ref
    sd = weights.random_uplift_state_dict(7, size, name, mode, 'old')
    assert [(k, v.shape) for k, v in sd.items()] == ref
    again = weights.random_uplift_state_dict(7, size, name, mode, 'new')          # time_rotation changes no weight
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    pos, first, second = arch.uplift_variant_layers(name, size, mode)
    depth = arch.UPLIFT_SIZES[size][1]
    assert len(pos) == (4 if mode == 'dynamic' else 0) and len(first) + len(second) == depth and len(second) == (0 if name == 'singlestage' else 4)
    assert all(p + '.attn.qkv.weight' in sd for p in pos + first + second)


def test_default_calls_return_what_they_always_did():
    for size in arch.UPLIFT_SIZES:
        assert arch.uplift_schema(size) == arch.uplift_variant_schema('connectstage', size, 'dynamic')
        assert arch.uplift_layers(size) == arch.uplift_variant_layers('connectstage', size, 'dynamic')
    with open(os.path.join(GOLDEN, 'uplift_schema.json')) as f:
        assert [(k, tuple(s)) for k, s in json.load(f)] == arch.uplift_schema('large')
    for size, sha in PARENT_BLOB_SHA256.items():
        old_call = weights.pack_uplift_blob(weights.random_uplift_state_dict(3, size), size)
        assert hashlib.sha256(old_call).hexdigest() == sha
        sd = weights.random_uplift_state_dict(3, size, 'connectstage', 'dynamic', 'new')
        assert weights.pack_uplift_blob(sd, size, name='connectstage', mode='dynamic', time_rotation='new') == old_call
        hdr = np.frombuffer(old_call[8:40], np.int32)
        assert hdr[6] == 0 and hdr[7] == 0


def test_blob_header_carries_the_variant():
    seen = set()
    for name, mode, rot in arch.uplift_variants():
        blob = weights.pack_uplift_blob(weights.random_uplift_state_dict(1, 'small', name, mode, rot), 'small', name, mode, rot)
        hdr = np.frombuffer(blob[8:40], np.int32)
        assert (arch.UPLIFT_NAMES[hdr[6] & 15], arch.UPLIFT_MODES[hdr[6] >> 4], arch.UPLIFT_ROTATIONS[hdr[7]]) == (name, mode, rot)
        pos, first, second = arch.uplift_variant_layers(name, 'small', mode)
        assert tuple(hdr[2:6]) == (len(pos), len(first), len(second), 13)
        seen.add((int(hdr[6]), int(hdr[7])))
    assert len(seen) == 18


def test_pack_refuses_another_variants_state_dict():
    stacked = weights.random_uplift_state_dict(1, 'small', 'connectstage', 'stacked')
    with pytest.raises(ValueError, match=r'firststage\.ball_embed\.fc1\.weight'):
        weights.pack_uplift_blob(stacked, 'small')                                      # packed as dynamic
    with pytest.raises(ValueError, match=r'firststage\.ball_embed\.fc1\.weight'):
        weights.pack_uplift_blob(stacked, 'small', 'connectstage', 'originalmethod')     # 41 columns where 28 are expected
    dynamic = weights.random_uplift_state_dict(1, 'small')
    with pytest.raises(ValueError, match=r'firststage\.table_embed\.fc1\.weight'):
        weights.pack_uplift_blob(dynamic, 'small', 'connectstage', 'stacked')            # a key stacked does not have
    with pytest.raises(ValueError, match=r'ball_embed\.fc1\.weight'):
        weights.pack_uplift_blob(weights.random_uplift_state_dict(1, 'small', 'singlestage', 'free'), 'small', 'multistage', 'dynamic')
    with pytest.raises(ValueError, match='large|shape'):
        weights.pack_uplift_blob(dynamic, 'large')


def test_get_model_raises_what_the_reference_raises():
    """Validation comes before the native library is loaded, so these need no GPU (uplifting/model.py:574-603, :311, :404)."""
    sd = weights.random_uplift_state_dict(1, 'small')
    with pytest.raises(ValueError, match='Unknown model name'):
        uplift.get_model('twostage', 'small', 'dynamic', 'new', state_dict=sd)
    with pytest.raises(ValueError, match='Unknown model size'):
        uplift.get_model('connectstage', 'tiny', 'dynamic', 'new', state_dict=sd)
    with pytest.raises(AssertionError):
        uplift.get_model('multistage', 'small', 'free', 'new', state_dict=sd)
    with pytest.raises(AssertionError):
        uplift.get_model('connectstage', 'small', 'free', 'new', state_dict=sd)
    with pytest.raises(AssertionError):
        uplift.get_model('singlestage', 'small', 'originalmethod', 'new', state_dict=sd)
    with pytest.raises(AssertionError):
        uplift.get_model('connectstage', 'small', 'dynamic', 'x', state_dict=sd)
    with pytest.raises(AssertionError):
        weights.random_uplift_state_dict(1, 'small', 'multistage', 'free')


def write_checkpoint(path, sd, name, size, mode, time_rotation, transform_mode):
    """A checkpoint file in the reference's format (uplifting/helper.py:371-391)."""
    import torch
    info = {'name': name, 'size': size, 'tabletoken_mode': mode, 'time_rotation': time_rotation, 'transform_mode': transform_mode,
            'randdet_prob': 0.0, 'randmiss_prob': 0.0, 'tablemiss_prob': 0.0}
    torch.save({'model_state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, 'identifier': 'unit-test', 'additional_info': info}, str(path))


def test_loader_picks_the_variant_from_additional_info(tmp_path, monkeypatch):
    """load_uplifting_model hands (name, size, tabletoken_mode, time_rotation) of the file to get_model with the file's weights and
    returns the file's transform_mode and the NormalizeImgCoords transform (the model itself is built in the GPU tests)."""
    sd = weights.random_uplift_state_dict(9, 'small', 'singlestage', 'stacked', 'old')
    path = tmp_path / 'model.pt'
    write_checkpoint(path, sd, 'singlestage', 'small', 'stacked', 'old', 'local')
    calls = []

    class Stub:
        def eval(self):
            return self

    def fake_get_model(name, size, mode, time_rotation, state_dict=None, **kw):
        calls.append((name, size, mode, time_rotation, weights.pack_uplift_blob(state_dict, size, name, mode, time_rotation), kw))
        return Stub()
    monkeypatch.setattr(uplift, 'get_model', fake_get_model)
    model, transform, transform_mode = inference.load_uplifting_model(str(path), max_len=40)
    assert isinstance(model, Stub) and transform_mode == 'local' and len(calls) == 1
    assert calls[0][:4] == ('singlestage', 'small', 'stacked', 'old') and calls[0][5]['max_len'] == 40
    assert calls[0][4] == weights.pack_uplift_blob(sd, 'small', 'singlestage', 'stacked', 'old')
    data = transform({'r_img': np.array([[1280.0, 720.0]]), 'table_img': np.array([[2560.0, 1440.0, 1.0]])})
    assert np.allclose(data['r_img'], 0.5) and np.allclose(data['table_img'], 1.0)
    # a file that names a combination the reference asserts against fails the same way
    write_checkpoint(path, sd, 'multistage', 'small', 'free', 'old', 'local')
    monkeypatch.undo()
    with pytest.raises(AssertionError):
        inference.load_uplifting_model(str(path))
