"""asm_autoaugment (csrc/autoaugment.hip) against tests/autoaugment_ref.py, the numpy restatement that
tests/test_autoaugment_cpu.py pins to the reference's source.  Outputs are integers (minus the channel means): every
comparison is exact.  The kernel has ONE code path for every size (an image lives in two L2-resident workspace planes,
never in LDS), so no size below sits on the other side of a switch."""
import numpy as np
import pytest
import torch

from tests import autoaugment_ref as R

pytestmark = pytest.mark.gpu


def _images(n, h, w, seed):
  """float32 with values below 0, above 255 and non-integers: the load's clip and truncation matter"""
  return np.random.default_rng(seed).uniform(-20.0, 275.0, size=(n, h, w, 3)).astype(np.float32)


def _table(specs, h, w):
  from assembled_cnn_amd import autoaugment as A
  return np.concatenate([A.descriptor(s, h, w) for s in specs])


def _run(images, table, subtract_mean):
  from assembled_cnn_amd import ops
  t = torch.from_numpy(table.view(np.uint8).copy()).cuda()
  return ops.autoaugment(torch.from_numpy(images).cuda(), t, subtract_mean).cpu().numpy()


def _check(images, specs, subtract_mean):
  h, w = images.shape[1:3]
  got = _run(images, _table(specs, h, w), subtract_mean)
  for k, s in enumerate(specs):
    want = R.augment(images[k], s, subtract_mean)
    assert np.array_equal(got[k], want), (k, s, int((got[k] != want).sum()))


def _all_specs(h, w, seed):
  """every op at levels 0..10, both signs where there is one, cutout centres spread over the image"""
  from assembled_cnn_amd import autoaugment as A
  rng = np.random.default_rng(seed)
  specs = []
  for name in A.OP_NAMES:
    for level in range(11):
      for negate in ((False, True) if name in A.SIGNED else (False,)):
        centre = (int(rng.integers(0, h)), int(rng.integers(0, w))) if name == 'Cutout' else ()
        specs.append((name,) + A.level_to_arg(name, level, negate) + centre)
  return specs


@pytest.mark.parametrize('subtract_mean', [False, True])
@pytest.mark.parametrize('h,w', [(37, 53), (8, 8)])
def test_every_op_every_level_in_one_diverging_batch(hip_lib, h, w, subtract_mean):
  """231 images with 231 different ops in one launch (workgroups diverge), then the same ops as SECOND slot after a
  different first one.  8 x 8: 64 pixels, so Equalize's step is 0 and Sharpness has a 6 x 6 interior."""
  specs = _all_specs(h, w, 1)
  assert len(specs) == 11 * 11 + 5 * 22
  images = _images(len(specs), h, w, 2)
  _check(images, [[s] for s in specs], subtract_mean)
  _check(images, [[specs[(k * 7 + 3) % len(specs)], s] for k, s in enumerate(specs)], subtract_mean)


@pytest.mark.parametrize('policy', ['imagenet', 'good'])
def test_every_sub_policy_with_both_slots_fired(hip_lib, policy):
  from assembled_cnn_amd import autoaugment as A
  h, w = 32, 48
  rng = np.random.default_rng(3)
  specs = []
  for k, sub in enumerate(A.POLICIES[policy]):
    pair = []
    for j, (name, _, level) in enumerate(sub):
      centre = (int(rng.integers(0, h)), int(rng.integers(0, w))) if name == 'Cutout' else ()
      pair.append((name,) + A.level_to_arg(name, level, (k + j) % 2 == 1) + centre)
    specs.append(pair)
  assert len(specs) == {'imagenet': 25, 'good': 95}[policy]
  _check(_images(len(specs), h, w, 4), specs, True)


def test_degenerate_images_and_pass_through(hip_lib):
  from assembled_cnn_amd import autoaugment as A
  h, w = 20, 24
  rng = np.random.default_rng(5)
  const = np.full((h, w, 3), 77.0, np.float32)
  one_channel = rng.uniform(0, 255, size=(h, w, 3)).astype(np.float32)
  one_channel[..., 1] = 200.25                                        # a channel with a single value
  two = np.where(rng.random((h, w, 3)) < 0.5, 10.0, 240.0).astype(np.float32)
  two_plane = np.where(rng.random((h, w, 1)) < 0.3, 3.0, 250.0).astype(np.float32).repeat(3, axis=2)
  ops5 = [(name,) + A.level_to_arg(name, 5 if name != 'Equalize' else 0, False) + ((7, 9) if name == 'Cutout' else ())
          for name in A.OP_NAMES]
  for base in (const, one_channel, two, two_plane):
    images = np.repeat(base[None], len(ops5), axis=0)
    _check(images, [[s] for s in ops5], False)
    _check(images, [[('Equalize',), s] for s in ops5], False)
  # op == 0 twice: trunc(clip(in)), and minus the means
  images = _images(3, h, w, 6)
  table = np.zeros(3, dtype=A.DESC_DTYPE)
  want = np.trunc(np.clip(images, 0, 255)).astype(np.float32)
  assert np.array_equal(_run(images, table, False), want)
  assert np.array_equal(_run(images, table, True), want - R.CHANNEL_MEANS)
  assert np.array_equal(_run(images, _table([[None, None]] * 3, h, w), False), want)


_MIX = [[('Equalize',), ('Rotate', 27.0)], [('Sharpness', 1.9), ('AutoContrast',)], [('ShearX', -0.3), ('Equalize',)],
        [('Color', 1.54), ('Contrast', 1.54)], [('TranslateY', 225.0), ('Solarize', 102)], [('Rotate', -30.0), ('Rotate', 12.0)],
        [('Cutout', 40, 100, 210), ('Posterize', 2)], [('Sharpness', 0.1), ('Sharpness', 0.64)]]


@pytest.mark.parametrize('n,side', [(8, 224), (2, 331)])
def test_recipe_sizes(hip_lib, n, side):
  """224 x 224 (the recipe) and 331 x 331 (odd, 328 KB per plane).  The kernel does not switch path by size."""
  _check(_images(n, side, side, 7), _MIX[:n], True)


def test_images_are_independent_and_runs_identical(hip_lib):
  h, w = 37, 53
  specs = _all_specs(h, w, 8)
  rng = np.random.default_rng(9)
  pairs = [[specs[int(rng.integers(len(specs)))], specs[int(rng.integers(len(specs)))]] for _ in range(16)]
  images = _images(16, h, w, 10)
  table = _table(pairs, h, w)
  a = _run(images, table, True)
  b = _run(images, table, True)
  assert np.array_equal(a, b)
  for k in range(16):
    alone = _run(images[k:k + 1], table[k:k + 1], True)
    assert np.array_equal(alone[0], a[k]), k
  # ... and in another order, among other neighbours
  perm = rng.permutation(16)
  assert np.array_equal(_run(images[perm], table[perm], True), a[perm])


def test_malformed_descriptors_are_defined(hip_lib):
  """Both are defined behaviour of the kernel (the host mirror refuses them first): an unknown op id passes the image
  through, a transform whose every sample lies outside the image gives the replace value everywhere."""
  from assembled_cnn_amd import autoaugment as A
  h, w = 19, 23
  images = _images(4, h, w, 11)
  table = np.zeros(4, dtype=A.DESC_DTYPE)
  table['slot'][0, 0]['op'] = 99
  table['slot'][1, 1]['op'] = -3
  table['slot'][2, 0]['op'] = A.OP_IDS['Posterize']
  table['slot'][2, 0]['a'] = 40                                        # a shift the kernel does not understand
  table['slot'][3, 0]['op'] = A.OP_IDS['Rotate']
  table['slot'][3, 0]['f'] = [0, 0, -5, 0, 0, 1e30]
  with pytest.raises(ValueError):
    A.validate(table[:1], h, w)
  with pytest.raises(ValueError):
    A.validate(table[2:3], h, w)
  got = _run(images, table, False)
  want = np.trunc(np.clip(images, 0, 255)).astype(np.float32)
  assert np.array_equal(got[:3], want[:3])
  assert np.array_equal(got[3], np.full((h, w, 3), 128.0, np.float32))


def test_preprocess_batch_end_to_end(hip_lib):
  from assembled_cnn_amd import autoaugment as A, input_pipeline as P, ops
  from oracle import input_oracle as IO
  rng = np.random.default_rng(12)
  imgs = [rng.integers(0, 256, size=(int(rng.integers(40, 300)), int(rng.integers(40, 300)), 3), dtype=np.uint8)
          for _ in range(6)]
  side = 64
  wins = [P.train_window(im.shape[0], im.shape[1], side, side, rng) for im in imgs]
  specs = [_MIX[0], _MIX[1], _MIX[2], _MIX[3], [('TranslateX', -20.0), ('Invert',)], [None, ('Cutout', 12, 5, 60)]]
  table = _table(specs, side, side)
  for sub in (True, False):
    out = P.preprocess_batch(imgs, True, 'cuda', image_size=side, windows=wins, subtract_mean=sub,
                             autoaugment_type='imagenet', augment=table).cpu().numpy()
    for k, (im, win) in enumerate(zip(imgs, wins)):
      resized = IO.preprocess_train_window(im, (win['crop_y'], win['crop_x'], win['crop_h'], win['crop_w'], win['flip']),
                                           side, side, subtract_mean=False)
      assert np.array_equal(out[k], R.augment(resized, specs[k], sub)), (sub, k)
  # sampled descriptors: the same seed gives the same batch, and it differs from the unaugmented one
  a = P.preprocess_batch(imgs, True, 'cuda', image_size=side, windows=wins, autoaugment_type='good',
                         rng=np.random.default_rng(1))
  b = P.preprocess_batch(imgs, True, 'cuda', image_size=side, windows=wins, autoaugment_type='good',
                         rng=np.random.default_rng(1))
  assert torch.equal(a, b)
  # no policy: bit-identical to the single launch as called today; evaluation ignores the policy name
  buf, tab = P.pack_batch(imgs, wins, side, side)
  plain = ops.resize_crop_flip(buf.cuda(), tab.cuda(), len(imgs), side, side, True)
  assert torch.equal(P.preprocess_batch(imgs, True, 'cuda', image_size=side, windows=wins, autoaugment_type=None), plain)
  ev = P.preprocess_batch(imgs, False, 'cuda', image_size=32)
  assert torch.equal(P.preprocess_batch(imgs, False, 'cuda', image_size=32, autoaugment_type='imagenet'), ev)
  with pytest.raises(ValueError, match='Invalid augmentation_name'):
    P.preprocess_batch(imgs, True, 'cuda', image_size=side, windows=wins, autoaugment_type='nope')


def test_the_launch_is_recorded_and_replayed_from_a_tape(hip_lib):
  from assembled_cnn_amd import ops
  h, w = 37, 53
  mix = _MIX[:6]
  images = _images(len(mix), h, w, 13)
  x = torch.from_numpy(images).cuda()
  t = torch.from_numpy(_table(mix, h, w).view(np.uint8).copy()).cuda()
  warm = ops.autoaugment(x, t, True)             # the workspace exists before the recording
  torch.cuda.synchronize()
  tape = ops.tape_begin()
  out = ops.autoaugment(x, t, True)
  assert ops.tape_end() == tape
  info = ops.tape_info(tape)
  assert (info['launches'], info['joins'], info['fills']) == (1, 0, 0), info
  torch.cuda.synchronize()
  assert torch.equal(out, warm)
  other = _images(len(mix), h, w, 14)
  x.copy_(torch.from_numpy(other))
  out.zero_()
  n0 = ops.L().asm_launch_count()
  ops.tape_replay(tape)
  assert ops.L().asm_launch_count() - n0 == 1
  torch.cuda.synchronize()
  got = out.cpu().numpy()
  for k, s in enumerate(mix):
    assert np.array_equal(got[k], R.augment(other[k], s, True)), k
  ops.tape_free(tape)
