"""AutoAugment without a GPU: tests/autoaugment_ref.py (the numpy restatement the HIP kernel is compared with) against
the reference's own source run under the shim (tests/golden/reference_autoaugment.*), known answers worked out by hand,
and the pure host side (assembled_cnn_amd/autoaugment.py: tables, arguments, sampling, descriptors, validation)."""
import json
import math
import os

import numpy as np
import pytest

from tests import autoaugment_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIGNED = ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY')


@pytest.fixture(scope='module')
def fixture():
  meta = json.load(open(os.path.join(GOLDEN, 'reference_autoaugment.json')))
  arrays = np.load(os.path.join(GOLDEN, 'reference_autoaugment.npz'))
  return meta, arrays


# ---- the restatement against the reference's source ---------------------------------------------------------------------
def test_ref_reproduces_every_recorded_op_output(fixture):
  meta, arrays = fixture
  assert meta['op_names'] == list(R.NAME_TO_FUNC)
  seen = set()
  for rec in meta['ops']:
    img = arrays['image/' + rec['image']]
    got = R.NAME_TO_FUNC[rec['name']](img, *rec['args'])
    assert got.dtype == np.uint8 and np.array_equal(got, arrays[rec['out']]), rec
    seen.add(rec['name'])
  assert seen == set(R.NAME_TO_FUNC) and len(meta['ops']) >= 150
  # the recorded outputs are not trivially the inputs
  changed = sum(not np.array_equal(arrays[r['out']], arrays['image/' + r['image']]) for r in meta['ops'])
  assert changed > len(meta['ops']) // 2


def _replay(meta, run, image):
  """distort_image_with_autoaugment (:767-903) over a stored list of uniform draws: the signs of every signed op of the
  table are drawn while the policy is built, then the sub-policy index, then per slot the apply draw (a fired cutout draws
  its centre row and column)."""
  table = meta['policies'][run['policy']]
  draws = iter(run['script'])
  by_key = {(e['name'], e['level'], e['u'] < 0.5): e['args'] for e in meta['level_to_arg']}
  args = [[tuple(by_key[(n, lv, next(draws) < 0.5 if n in SIGNED else False)]) for (n, p, lv) in sub] for sub in table]
  selected = int(math.floor(next(draws) * len(table)))
  fired = []
  for (n, p, lv), a in zip(table[selected], args[selected]):
    f = bool(np.floor(np.float32(next(draws)) + np.float32(p)) >= 1)
    fired.append(f)
    if f:
      if n == 'Cutout':
        a = a + (int(math.floor(next(draws) * image.shape[0])), int(math.floor(next(draws) * image.shape[1])))
      image = R.NAME_TO_FUNC[n](image, *a)
  assert next(draws, None) is None, 'the reference drew more often'
  return selected, fired, image


def test_ref_reproduces_every_scripted_end_to_end_run(fixture):
  meta, arrays = fixture
  assert len(meta['runs']) >= 6
  any_skipped = False
  for run in meta['runs']:
    selected, fired, out = _replay(meta, run, arrays['image/' + run['image']])
    assert (selected, fired) == (run['selected'], run['fired']), run['policy']
    assert np.array_equal(out, arrays[run['out']]), (run['policy'], selected)
    any_skipped |= not all(fired)
  assert any_skipped and any(all(r['fired']) for r in meta['runs'])
  assert len({(r['policy'], r['selected']) for r in meta['runs']}) >= 6


# ---- the host module against the recorded tables and arguments ------------------------------------------------------------
def test_policies_and_level_to_arg_equal_the_reference(fixture):
  from assembled_cnn_amd import autoaugment as A
  meta, _ = fixture
  assert sorted(A.POLICIES) == sorted(meta['policies'])
  for name, table in meta['policies'].items():
    assert [[list(op) for op in sub] for sub in A.POLICIES[name]] == table, name
  assert list(A.OP_NAMES) == meta['op_names'] and A.OP_IDS['AutoContrast'] == 1 and A.OP_IDS['Cutout'] == 16
  assert len(meta['level_to_arg']) == 16 * 11 * 2
  for e in meta['level_to_arg']:
    got = A.level_to_arg(e['name'], e['level'], negate=e['u'] < 0.5)
    assert list(got) == e['args'] and [type(v) for v in got] == [type(v) for v in e['args']], e
    assert e['draws'] == (1 if e['name'] in A.SIGNED else 0)


# ---- known answers, worked out by hand ----------------------------------------------------------------------------------
def _rand(h, w, seed=0):
  return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_contrast_blends_toward_the_pixel_count_over_256():
  """16 x 16 = 256 pixels: the histogram sums to 256, "mean" = 256 / 256 = 1, so the degenerate image is the constant 1
  whatever the image holds.  factor 0.5: 1 + 0.5 * (v - 1), truncated."""
  img = _rand(16, 16)
  got = R.contrast(img, 0.5)
  assert np.array_equal(got, np.floor(1 + 0.5 * (img.astype(np.float64) - 1)).astype(np.uint8))
  assert np.array_equal(R.contrast(np.full((16, 16, 3), 200, np.uint8), 0.5), np.full((16, 16, 3), 100, np.uint8))
  # 32 x 16 pixels -> the constant 2
  assert np.array_equal(R.contrast(np.full((32, 16, 3), 201, np.uint8), 0.5), np.full((32, 16, 3), 101, np.uint8))


def test_equalize_known_answers():
  # 8 x 8: at most 64 pixels, (64 - last bin) // 255 == 0 -> unchanged
  img = _rand(8, 8, 1)
  assert np.array_equal(R.equalize(img), img)
  # 32 x 32 = 1024 pixels per channel, values 10 (x 512), 20 (x 256), 30 (x 256): step = (1024 - 256) // 255 = 3;
  # lut[v] = (pixels below v + 1) // 3 clipped: lut[10] = 0, lut[20] = 513 // 3 = 171, lut[30] = 769 // 3 = 256 -> 255
  ch = np.concatenate([np.full(512, 10), np.full(256, 20), np.full(256, 30)]).astype(np.uint8)
  img = np.stack([np.random.default_rng(c).permutation(ch).reshape(32, 32) for c in range(3)], axis=2)
  want = np.select([img == 10, img == 20, img == 30], [0, 171, 255]).astype(np.uint8)
  assert np.array_equal(R.equalize(img), want)
  # one channel constant: (1024 - 1024) // 255 == 0 keeps that channel, the others change
  img2 = img.copy()
  img2[..., 1] = 99
  got = R.equalize(img2)
  assert np.array_equal(got[..., 1], img2[..., 1]) and np.array_equal(got[..., 0], want[..., 0])


def test_autocontrast_known_answers():
  img = _rand(5, 7, 2)
  img[..., 2] = 131                                        # hi == lo: unchanged
  img[0, 0, 0], img[0, 1, 0] = 0, 255                      # already full range: scale 1, offset 0
  got = R.autocontrast(img)
  assert np.array_equal(got[..., 2], img[..., 2]) and np.array_equal(got[..., 0], img[..., 0])
  ramp = np.zeros((1, 3, 3), np.uint8)
  ramp[0, :, 0] = [50, 100, 150]                           # scale 2.55, offset -127.5 -> 0, 127.5, 255
  assert R.autocontrast(ramp)[0, :, 0].tolist() == [0, 127, 255]


def test_the_four_blend_branches():
  a = np.array([[[0, 100, 250]]], np.uint8)
  b = np.array([[[200, 50, 10]]], np.uint8)
  assert np.array_equal(R.blend(a, b, 0.0), a) and np.array_equal(R.blend(a, b, 1.0), b)
  assert R.blend(a, b, 0.25).reshape(-1).tolist() == [50, 87, 190]          # 87.5 truncates; nothing to clip
  assert R.blend(a, b, 1.5).reshape(-1).tolist() == [255, 25, 0]            # 300 and -110 clip, then truncate
  assert R.blend(a, b, 1.9).reshape(-1).tolist() == [255, 5, 0]             # float32(1.9) * -50 rounds to -95 exactly
  # brightness / color are blends from a degenerate image
  assert R.brightness(a, 1.9).reshape(-1).tolist() == [0, 190, 255]
  white = np.full((2, 2, 3), 255, np.uint8)
  assert R.rgb_to_grayscale(white).tolist() == [[255, 255], [255, 255]]      # 0.9999 * 255.5 = 255.47 -> 255
  assert np.array_equal(R.color(white, 0.3), white)


def test_sharpness_keeps_the_border_ring():
  img = _rand(9, 11, 3)
  for factor in (0.1, 0.64, 1.9):
    got = R.sharpness(img, factor)
    assert np.array_equal(got[0], img[0]) and np.array_equal(got[-1], img[-1])
    assert np.array_equal(got[:, 0], img[:, 0]) and np.array_equal(got[:, -1], img[:, -1])
    assert not np.array_equal(got[1:-1, 1:-1], img[1:-1, 1:-1])
  flat = np.full((5, 5, 3), 91, np.uint8)                  # the smoothed constant is 91 * (8/13 + 5/13) -> 91 or 90.99..
  assert np.abs(R.sharpness(flat, 0.5).astype(int) - 91).max() <= 1
  assert np.array_equal(R.sharpness(img[:2], 0.3), img[:2])                  # no interior at all


def test_geometric_known_answers():
  img = _rand(24, 40, 4)
  assert np.array_equal(R.rotate(img, 0.0), img) and np.array_equal(R.rotate(img, -0.0), img)
  assert np.array_equal(R.translate_x(img, 0.0), img) and np.array_equal(R.translate_y(img, 0.0), img)
  assert np.array_equal(R.shear_x(img, 0.0), img)
  t = R.translate_x(img, 3.0)                              # output x reads input x + 3: content moves left
  assert np.array_equal(t[:, :-3], img[:, 3:]) and (t[:, -3:] == 128).all()
  t = R.translate_x(img, -3.0)
  assert np.array_equal(t[:, 3:], img[:, :-3]) and (t[:, :3] == 128).all()
  t = R.translate_y(img, 250.0)
  assert (t == 128).all()
  sq = _rand(17, 17, 5)                                    # a square rotates onto itself by 90 degrees
  r = R.rotate(sq, 90.0)
  assert np.array_equal(r, np.rot90(sq, 1)) or np.array_equal(r, np.rot90(sq, 3))
  c = R.cutout(img, 4, 2, 38)
  assert (c[0:6, 34:40] == 128).all() and np.array_equal(c[6:], img[6:]) and np.array_equal(c[:, :34], img[:, :34])
  assert np.array_equal(R.cutout(img, 0, 5, 5), img)       # pad size 0: nothing is filled


def test_posterize_and_solarize_edge_arguments():
  img = _rand(6, 6, 6)
  assert not R.posterize(img, 0).any()                     # bits = 0 shifts by 8: defined as 0
  assert np.array_equal(R.posterize(img, 8), img) and np.array_equal(R.posterize(img, 4), img & 0xf0)
  assert np.array_equal(R.solarize(img, 256), img)         # compared as int: every pixel is kept
  assert np.array_equal(R.solarize(img, 0), 255 - img)
  assert np.array_equal(R.solarize_add(img, 110), np.where(img < 128, np.minimum(img.astype(int) + 110, 255), img))
  assert np.array_equal(R.invert(img), 255 - img)
  assert np.array_equal(R.to_uint8(np.array([-3.5, 0.9, 254.99, 255.0, 300.0], np.float32)), [0, 0, 254, 255, 255])


# ---- sampling, descriptors, validation ------------------------------------------------------------------------------------
def test_sample_probabilities_indices_and_seed():
  from assembled_cnn_amd import autoaugment as A
  d, idx = A.sample('imagenet', 2000, 224, 224, np.random.default_rng(0), return_index=True)
  assert d.dtype == A.DESC_DTYPE and d.shape == (2000,) and idx.shape == (2000,)
  ops = d['slot']['op']
  # ('Equalize', 0.0, 7), ('Equalize', 0.8, 8) holds the table's only probability 0.0: its first slot never fires
  assert A.POLICIES['imagenet'].index([('Equalize', 0.0, 7), ('Equalize', 0.8, 8)]) == 12
  assert set(idx.tolist()) == set(range(25))
  assert (idx == 12).sum() > 40 and (ops[idx == 12, 0] == 0).all()
  for k, sub in enumerate(A.POLICIES['imagenet']):
    for s, (op, prob, level) in enumerate(sub):
      fired = ops[idx == k, s] != 0
      if prob == 1.0:
        assert fired.all(), (k, s)
      elif prob == 0.0:
        assert not fired.any(), (k, s)
      assert set(ops[idx == k, s].tolist()) <= {0, A.OP_IDS[op]}
  # 0.4 .. 0.8 elsewhere: both outcomes occur, signs go both ways
  assert 0.4 < (ops != 0).mean() < 0.8
  rot = d['slot'][ops == A.OP_IDS['Rotate']]['f'][:, 1]
  assert (rot > 0).any() and (rot < 0).any()
  assert np.array_equal(d, A.sample('imagenet', 2000, 224, 224, np.random.default_rng(0)))
  assert not np.array_equal(d, A.sample('imagenet', 2000, 224, 224, np.random.default_rng(1)))
  g = A.sample('good', 2000, 64, 48, np.random.default_rng(2))
  cut = g['slot'][g['slot']['op'] == A.OP_IDS['Cutout']]
  assert len(cut) and ((cut['b'] >> 16) < 64).all() and ((cut['b'] & 0xffff) < 48).all()
  t = A.sample('test', 50, 32, 32, np.random.default_rng(3))
  assert (t['slot']['op'] == [A.OP_IDS['TranslateX'], A.OP_IDS['Equalize']]).all()
  for name, n in (('imagenet', d), ('good', g), ('test', t)):
    A.validate(n, *((224, 224) if name == 'imagenet' else (64, 48) if name == 'good' else (32, 32)))


def test_descriptor_layout_and_validation():
  import ctypes
  from assembled_cnn_amd import autoaugment as A, lib
  assert A.DESC_DTYPE.itemsize == ctypes.sizeof(lib.AugmentDesc) == 80 and ctypes.sizeof(lib.AugmentOp) == 40
  d = A.descriptor([('Posterize', 3), ('Rotate', 30.0)], 24, 40)
  raw = d.view(np.uint8).reshape(-1)
  c = lib.AugmentDesc.from_buffer_copy(raw.tobytes())
  assert (c.slot[0].op, c.slot[0].a, c.slot[1].op) == (5, 5, 4)
  want = R.rotate_coeffs(30.0, 24, 40)
  assert [c.slot[1].f[i] for i in range(6)] == [float(v) for v in want]
  assert abs(c.slot[1].f[0] - math.cos(math.pi / 6)) < 1e-7 and abs(c.slot[1].f[3] - 0.5) < 1e-7
  d = A.descriptor([('Cutout', 40, 3, 7), ('SolarizeAdd', 33)], 24, 40)
  s = d['slot'][0]
  assert (s['a'].tolist(), s['b'].tolist()) == ([40, 33], [(3 << 16) | 7, 128])
  assert A.descriptor([('TranslateX', 25.0)], 8, 8)['slot'][0, 0]['f'].tolist() == [1, 0, 25, 0, 1, 0]
  assert A.descriptor([('ShearY', -0.3)], 8, 8)['slot'][0, 0]['f'].tolist() == [1, 0, 0, float(np.float32(-0.3)), 1, 0]
  assert A.descriptor([('Color', 1.54)], 8, 8)['slot'][0, 0]['f'][0] == np.float32(1.54)
  assert (A.descriptor([], 8, 8)['slot']['op'] == 0).all() and (A.descriptor([None, ('Invert',)], 8, 8)['slot']['op'] == [0, 3]).all()
  for name in A.OP_NAMES:       # every descriptor that descriptor() builds passes validation
    for level in range(11):
      extra = (2, 3) if name == 'Cutout' else ()
      A.validate(A.descriptor([(name,) + A.level_to_arg(name, level, True) + extra], 24, 40), 24, 40)
  for bad in ([('Sharpen', 1.0)], [('Posterize', 9)], [('Posterize', 2.5)], [('Solarize', 257)], [('Cutout', 3, 24, 0)],
              [('Cutout', 3, 0, 40)], [('Color', float('nan'))], [('Color', -0.5)], [('Rotate', float('inf'))],
              [('Invert', 1)], [('Rotate',)], [('Invert',)] * 3):
    with pytest.raises(ValueError):
      A.descriptor(bad, 24, 40)
  with pytest.raises(ValueError, match='Invalid augmentation_name: nope'):
    A.sample('nope', 1, 8, 8, np.random.default_rng(0))
  for name, level in (('Rotate', 11), ('Rotate', -1), ('Rotate', 2.5), ('Nope', 3)):
    with pytest.raises(ValueError):
      A.level_to_arg(name, level)
  good = A.descriptor([('Posterize', 3), ('Rotate', 30.0)], 24, 40)
  for field, value in (('op', 17), ('op', -1), ('a', 9)):
    broken = good.copy()
    broken['slot'][0, 0][field] = value
    with pytest.raises(ValueError):
      A.validate(broken, 24, 40)
  broken = good.copy()
  broken['slot'][0, 1]['f'][2] = np.nan
  with pytest.raises(ValueError):
    A.validate(broken, 24, 40)
  with pytest.raises(ValueError):
    A.validate(A.descriptor([('Cutout', 3, 20, 30)], 24, 40), 16, 16)       # centre outside a smaller image
  with pytest.raises(ValueError):
    A.descriptor([], 40000, 8)


def test_preprocess_batch_refuses_an_unknown_policy():
  from assembled_cnn_amd import input_pipeline as P
  with pytest.raises(ValueError, match='Invalid augmentation_name: nope'):
    P.preprocess_batch([np.zeros((8, 8, 3), np.uint8)], True, 'cpu', autoaugment_type='nope')
