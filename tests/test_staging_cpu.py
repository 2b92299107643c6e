"""staging.Staging, the one grow-only host buffer type of the input path, and RecordDataset's upload through an instance of
its own: storage that is never shared, the grow rule, where fill puts the bytes, and the payload spans of a batch.  No GPU."""
import numpy as np
import torch

from assembled_cnn_amd import records, staging
from tests import jpeg_parse_cases as cases
from tests.test_jpeg_device_parse_cpu import NAMES


def _capacity(t: torch.Tensor) -> int:
  return t.untyped_storage().nbytes()


def _base(t: torch.Tensor) -> int:
  return t.untyped_storage().data_ptr()


def test_two_instances_never_share_storage():
  a, b = staging.Staging(), staging.Staging()
  one = np.full(64, 1, np.uint8)
  two = np.full(64, 2, np.uint8)
  fa = a.fill(64, [one], [0], False)
  fb = b.fill(64, [two], [0], False)
  fd = staging.fill(64, [two], [0], False)            # the module's default instance is a third one
  assert len({_base(fa), _base(fb), _base(fd)}) == 3
  assert fa.tolist() == [1] * 64 and fb.tolist() == [2] * 64      # b's fill did not land in a's buffer
  region_a, region_b = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
  a.stage_into(region_a, [one], [0])
  b.stage_into(region_b, [two], [0])
  assert region_a.tolist() == [1] * 64 and region_b.tolist() == [2] * 64
  assert staging.fill.__self__ is staging.stage_into.__self__ and isinstance(staging.fill.__self__, staging.Staging)


def test_buffer_is_reused_and_grows_by_the_rule():
  s = staging.Staging()
  first = s.fill(1000, [], [], False)
  assert first.numel() == 1000 and _capacity(first) == int(1000 * 1.25) + 4096 == 5346
  for smaller in (10, 1000, 5346):                      # up to the capacity itself: no new allocation
    again = s.fill(smaller, [], [], False)
    assert again.numel() == smaller and _base(again) == _base(first) and _capacity(again) == 5346
  grown = s.fill(5347, [], [], False)
  assert grown.numel() == 5347 and _capacity(grown) == int(5347 * 1.25) + 4096 == 10779
  assert _base(s.fill(6000, [], [], False)) == _base(grown)       # and that one is kept


def test_fill_places_each_array_at_its_offset_and_leaves_the_padding():
  s = staging.Staging()
  rng = np.random.default_rng(5)
  image = rng.integers(0, 256, (3, 4, 3), dtype=np.uint8)                       # 36 bytes, three-dimensional
  strided = rng.integers(0, 256, 66, dtype=np.uint8)[::2]                       # 33 bytes, not contiguous
  arrays = [rng.integers(0, 256, 5, dtype=np.uint8), image, rng.integers(0, 256, 16, dtype=np.uint8),
            rng.integers(0, 256, 1, dtype=np.uint8), strided]
  offsets, total = staging.slot_layout([a.size for a in arrays])
  assert offsets.tolist() == [0, 16, 64, 80, 96] and total == 144
  s.fill(total, [np.full(total, 0xEE, np.uint8)], [0], False)                   # what an earlier batch left behind
  got = s.fill(total, arrays, offsets, False).numpy()
  want = np.full(total, 0xEE, np.uint8)
  for a, o in zip(arrays, offsets):
    want[o:o + a.size] = a.reshape(-1)
  assert np.array_equal(got, want)
  assert (got[5:16] == 0xEE).all() and (got[52:64] == 0xEE).all() and (got[81:96] == 0xEE).all() and (got[129:] == 0xEE).all()
  # a later, shorter array in a slot touches its own bytes alone
  got = s.fill(total, [np.zeros(2, np.uint8)], [16], False).numpy()
  want[16:18] = 0
  assert np.array_equal(got, want)
  region = torch.zeros(total, dtype=torch.uint8)
  s.stage_into(region, arrays, offsets)
  want[16:52] = image.reshape(-1)
  assert np.array_equal(region.numpy(), want)


def test_record_upload_keeps_its_slots_and_spans(tmp_path):
  fx = cases.load()
  files = [fx[n][0] for n in NAMES]
  payloads = [records.encode_example({'image/encoded': [f], 'image/filename': [n.encode()],
                                      'image/class/label': np.array([i])}) for i, (n, f) in enumerate(zip(NAMES, files))]
  path = str(tmp_path / 'validation-00000-of-00001')
  records.write_records(path, payloads)
  ds = records.RecordDataset([path], False, 5, 1, verify='host', device='cpu', keep_payloads=True)
  seen = batches = capacity = 0
  for batch in ds:                                      # the buffer is refilled by the next batch: look at each in turn
    n = len(batch.encoded)
    mine, data = payloads[seen:seen + n], files[seen:seen + n]
    buf, where = batch.payloads
    offsets, total = staging.slot_layout([len(p) for p in mine])
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.numel() == total
    assert where.dtype == np.int64 and where.shape == (n, 2)
    host = buf.numpy()
    for k in range(n):
      assert host[offsets[k]:offsets[k] + len(mine[k])].tobytes() == mine[k]          # the whole record in its slot
      o, ln = int(where[k, 0]), int(where[k, 1])
      assert host[o:o + ln].tobytes() == data[k] == batch.encoded[k].tobytes()
      assert o == offsets[k] + mine[k].find(data[k]) and ln == len(data[k])
    if total > capacity:                                # the dataset's device buffer: grow-only, by the same rule
      capacity = int(total * 1.25) + 4096
    assert _capacity(buf) == capacity
    seen += n
    batches += 1
  assert seen == 8 and batches == 2
  assert not hasattr(ds, '_host') and not hasattr(ds, '_uploaded')
  assert isinstance(ds._staging, staging.Staging) and ds._staging is not staging.fill.__self__
