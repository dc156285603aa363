"""Writes tests/golden/jpeg.json: SHA-256 digests, from Pillow itself, of the 360 x 640 4:2:0 quality-90 frame of tests/jpeg_cases.py
(`big_case`: seeded ramps plus noise, generated where the test runs) -- of the encoded stream and of Pillow's decode of it -- with the
versions that produced them.  Run where Pillow is installed; the tests need Pillow too (they encode the frame) and compare both digests.

    python tests/golden/make_jpeg_golden.py"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import jpeg_cases as J  # noqa: E402


def main():
    import PIL
    from PIL import features
    blob = J.big_case()
    out = {"frame": f"{J.BIG[0]}x{J.BIG[1]} subsampling=2 quality=90 content=photo", "pillow": PIL.__version__, "libjpeg": features.version("jpg"),
           "pixels_sha256": J.sha256(J.pixels(*J.BIG, "photo")), "stream_bytes": len(blob), "stream_sha256": J.sha256(blob), "decoded_sha256": J.sha256(J.pillow(blob))}
    path = HERE / "jpeg.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(path, out)


if __name__ == "__main__":
    main()
