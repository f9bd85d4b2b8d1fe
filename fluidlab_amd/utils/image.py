"""PNG output with the standard library only (zlib, struct): the package has no imaging dependency."""
import struct
import zlib

import numpy as np

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(rgb, level=6):
    """uint8 [H, W, 3] (RGB) or [H, W, 4] (RGBA) -> the bytes of an 8-bit PNG (filter 0 on every row)"""
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'encode_png: a uint8 array [H, W, 3] or [H, W, 4] is needed, got {a.dtype} {a.shape}')
    H, W, ch = a.shape
    rows = np.empty((H, 1 + W * ch), np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = a.reshape(H, W * ch)
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 2 if ch == 3 else 6, 0, 0, 0)
    return PNG_SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_png(path, rgb):
    with open(path, 'wb') as f:
        f.write(encode_png(rgb))
