"""Host half of the device PNG encoder (ops.png_deflate, DESIGN.md "PNG encode on the device"): the device hands over the finished
zlib stream of the filtered rows; what is left is the container -- signature, IHDR, one IDAT with its CRC-32, IEND."""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_COLOUR_TYPE = {3: 2, 1: 0}          # RGB / greyscale, 8 bits per sample


def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(tag)))


def frame(zlib_bytes, H, W, C):
    """The PNG file of an H x W image with C channels whose zlib stream (filter type byte + residuals per row) is `zlib_bytes`."""
    if C not in _COLOUR_TYPE:
        raise ValueError(f"PNG framing of {C} channels: RGB (3) and greyscale (1) only")
    ihdr = struct.pack(">IIBBBBB", W, H, 8, _COLOUR_TYPE[C], 0, 0, 0)
    return b"".join((SIGNATURE, _chunk(b"IHDR", ihdr), _chunk(b"IDAT", bytes(zlib_bytes)), _chunk(b"IEND", b"")))


def write(zlib_bytes, H, W, C, path):
    with open(path, "wb") as f:
        f.write(frame(zlib_bytes, H, W, C))
