"""Writes the glyph atlas that aocr.GlyphAtlas.default() loads (torch-attention-ocr_amd/aocr/glyph_atlas.txt): 0-9 a-z at gh = 32 in up
to three faces, rendered through Pillow from fonts found on this machine (aocr.synth_lines.render_atlas: every face at the largest size
whose ink fits 32 rows).  The file is text (GlyphAtlas.save: one character per pixel, 16 ink levels) and
records the font names and pixel sizes.  Needs Pillow; no GPU.

    python tools/make_glyph_atlas.py [font.ttf ...]        # default: the first serif, sans and monospace DejaVu / Liberation face found
"""
import glob
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "torch-attention-ocr_amd"))
WANTED = ("DejaVuSans.ttf", "DejaVuSerif.ttf", "DejaVuSansMono.ttf", "LiberationSans-Regular.ttf", "LiberationSerif-Regular.ttf",
          "LiberationMono-Regular.ttf")
DIRS = ("/usr/share/fonts", "/usr/local/share/fonts", os.path.expanduser("~/.fonts"))
MAX_BYTES = 64 * 1024


def find_fonts():
    have = {}
    for d in DIRS:
        for p in sorted(glob.glob(os.path.join(d, "**", "*.ttf"), recursive=True)):
            have.setdefault(os.path.basename(p), p)
    return [have[n] for n in WANTED if n in have][:3]


def main():
    paths = sys.argv[1:] or find_fonts()
    if not paths:
        sys.exit("no font found: pass TrueType files on the command line")
    from aocr.synth_lines import DEFAULT_ATLAS, DEFAULT_CHARS, GlyphAtlas, render_atlas       # imports the package: libaocr.so must be built
    pixels, advance, names = render_atlas(paths[:3], 32, DEFAULT_CHARS)
    GlyphAtlas(pixels, advance, names).save(DEFAULT_ATLAS)
    size = os.path.getsize(DEFAULT_ATLAS)
    print(f"{DEFAULT_ATLAS}: {pixels.shape} from {names}, {size} bytes")
    if size > MAX_BYTES:
        sys.exit(f"the atlas must stay under {MAX_BYTES} bytes: use fewer faces")


if __name__ == "__main__":
    main()
