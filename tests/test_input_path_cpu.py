"""Host plumbing of the input path: the device tables have ONE Python declaration (the ctypes structs of lib.py) whose
layout is pinned here against include/asm_hip.h, decoded arrays and encoded files share one slot layout, and
preprocess_batch's single body equals the host-only route (pack_batch + ops.resize_crop_flip)."""
import numpy as np
import pytest
import torch

I8, I4, F4, U1, U2 = '<i8', '<i4', '<f4', 'u1', '<u2'


def _ints(names, first, base=I4):
  size = np.dtype(base).itemsize
  return [(n, first + size * k, base, ()) for k, n in enumerate(names.split())]


# struct name in lib.py -> (sizeof, [(field, byte offset, base type or nested struct, array shape)]), read off the typedefs
# of include/asm_hip.h (asm_image_desc, asm_augment_op, asm_augment_desc, asm_jpeg_desc, asm_jpeg_huff, asm_jpeg_tables,
# asm_jpeg_interval), NOT off the Python classes
LAYOUT = {
    'ImageDesc': (56, [('src_offset', 0, I8, ())] +
                  _ints('Hs Ws crop_y crop_x crop_h crop_w resize_h resize_w out_y out_x flip reserved', 8)),
    'AugmentOp': (40, _ints('op a b reserved', 0) + [('f', 16, F4, (6,))]),
    'AugmentDesc': (80, [('slot', 0, 'AugmentOp', (2,))]),
    'JpegDesc': (96, _ints('scan_offset scan_bytes coef_offset plane_offset dst_offset', 0, I8) +
                 _ints('width height ncomp hs vs mcus_x mcus_y restart_interval first_interval n_intervals', 40) +
                 [('qsel', 80, U1, (4,)), ('dcsel', 84, U1, (4,)), ('acsel', 88, U1, (4,)), ('reserved', 92, I4, ())]),
    'JpegHuff': (272, [('bits', 0, U1, (16,)), ('vals', 16, U1, (256,))]),
    'JpegTables': (1600, [('quant', 0, U2, (4, 64)), ('dc', 512, 'JpegHuff', (2,)), ('ac', 1056, 'JpegHuff', (2,))]),
    'JpegInterval': (32, _ints('image first_mcu n_mcus rst', 0) + _ints('byte_begin byte_end', 16, I8)),
}


@pytest.mark.parametrize('name', sorted(LAYOUT))
def test_table_dtype_layout_matches_the_header(name):
  from assembled_cnn_amd import lib
  size, fields = LAYOUT[name]
  dt = np.dtype(getattr(lib, name))
  assert dt.itemsize == size
  assert list(dt.names) == [f[0] for f in fields]
  for field, offset, base, shape in fields:
    ftype, at = dt.fields[field][:2]
    dims = ()
    while ftype.subdtype is not None:       # an array of arrays (uint16 quant[4][64]) nests: collect every dimension
      ftype, dims = ftype.subdtype[0], dims + ftype.subdtype[1]
    want = np.dtype(getattr(lib, base)) if base in LAYOUT else np.dtype(base)
    assert (at, ftype, dims) == (offset, want, shape), (name, field)


def test_module_dtypes_are_the_struct_dtypes():
  from assembled_cnn_amd import autoaugment, input_pipeline, jpeg, lib
  for got, struct in ((input_pipeline._DESC_DTYPE, lib.ImageDesc), (autoaugment.OP_DTYPE, lib.AugmentOp),
                      (autoaugment.DESC_DTYPE, lib.AugmentDesc), (jpeg.DESC_DTYPE, lib.JpegDesc),
                      (jpeg.HUFF_DTYPE, lib.JpegHuff), (jpeg.TABLES_DTYPE, lib.JpegTables),
                      (jpeg.INTERVAL_DTYPE, lib.JpegInterval)):
    assert got == np.dtype(struct)


def images():
  """three decoded images: an odd size, one that is no multiple of 16 bytes wide, one whose slot needs no padding"""
  rng = np.random.default_rng(11)
  return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((17, 23), (40, 31), (64, 64))]


def test_decoded_arrays_get_pack_batch_slots():
  from assembled_cnn_amd import input_pipeline as P, jpeg
  imgs = images()
  pk = jpeg.pack(imgs)
  assert pk.dev_index == [] and pk.host_begin == 0
  assert pk.sizes == [im.shape[:2] for im in imgs]
  wins = [dict(crop_y=0, crop_x=0, crop_h=h, crop_w=w, resize_h=h, resize_w=w, out_y=0, out_x=0, flip=0) for h, w in pk.sizes]
  buf, table = P.pack_batch(imgs, wins, 16, 16)
  assert pk.offsets.tolist() == table.numpy().view(P._DESC_DTYPE)['src_offset'].tolist() == [0, 1184, 1184 + 3728]
  assert pk.total_bytes == buf.numel() == 1184 + 3728 + 64 * 64 * 3
  packed = buf.numpy().copy()
  got = jpeg.decode_packed(pk, 'cpu')[0].numpy()
  for im, o in zip(imgs, pk.offsets):
    assert np.array_equal(got[o:o + im.size], im.reshape(-1)) and np.array_equal(packed[o:o + im.size], im.reshape(-1))


def check_preprocess_batch_equals_the_pack_batch_route(device, subtract_mean):
  """preprocess_batch (jpeg.pack -> decode_packed -> resize) against pack_batch's buffer and table through
  ops.resize_crop_flip, same windows: an evaluation window, a training window with a flip, an identity window"""
  from assembled_cnn_amd import input_pipeline as P, ops
  imgs, side = images(), 32
  wins = [P.eval_window(17, 23, side, side), dict(P.train_window(40, 31, side, side, np.random.default_rng(3)), flip=1),
          dict(crop_y=0, crop_x=0, crop_h=64, crop_w=64, resize_h=64, resize_w=64, out_y=0, out_x=0, flip=0)]
  buf, table = P.pack_batch(imgs, wins, side, side)
  want = ops.resize_crop_flip(buf.clone().to(device), table.to(device), len(imgs), side, side, subtract_mean)
  got = P.preprocess_batch(imgs, False, device, image_size=side, windows=wins, subtract_mean=subtract_mean)
  assert got.shape == want.shape == (3, side, side, 3) and got.dtype == want.dtype == torch.float32
  assert torch.equal(got, want)
  # the identity window is the image's top-left corner, the flipped one is not left as it was
  corner = torch.from_numpy(imgs[2][:side, :side].astype(np.float32))
  if subtract_mean:
    corner = corner - torch.tensor([123.68, 116.78, 103.94])
  assert torch.equal(got[2].cpu(), corner)
  unflipped = P.preprocess_batch(imgs, False, device, image_size=side, windows=[dict(w, flip=0) for w in wins],
                                 subtract_mean=subtract_mean)
  assert torch.equal(unflipped[0], got[0]) and not torch.equal(unflipped[1], got[1])


@pytest.mark.parametrize('subtract_mean', [True, False])
def test_preprocess_batch_equals_the_pack_batch_route(cpu_double, subtract_mean):
  check_preprocess_batch_equals_the_pack_batch_route('cpu', subtract_mean)
