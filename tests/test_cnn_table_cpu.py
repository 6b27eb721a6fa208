"""CPU: what the CNN layer table (csrc/cnn.h) feeds -- the parameter layout, the gradient buckets, the BatchNorm state count and the
workspace carve-up -- for the five BASELINE.json configurations in both compute modes.  The expected values are those the library gave
while every one of these places still kept a hand-written copy of the layer shapes: a change of the table, or of the order or size of a
workspace region, shows here without a GPU."""
import ctypes as C

import pytest

# batch_size, img_h, max_img_w, enc_hidden, enc_layers, dec_layers, max_beam (vocab 39, emb 20, input feed, max_decoder_l 50)
CONFIGS = {
    "c1": (1, 32, 100, 256, 1, 2, 1), "c2": (64, 32, 100, 256, 1, 2, 1), "c3": (256, 32, 256, 256, 1, 2, 1),
    "c4": (64, 32, 800, 256, 1, 2, 1), "c5": (256, 128, 1024, 512, 2, 2, 5)}
WORKSPACE = {  # aocr_workspace_bytes: (fp32, bf16)
    "c1": (60117248, 149918208),
    "c2": (491074048, 709095936),
    "c3": (3117291264, 4159103744),
    "c4": (1965910784, 2665622272),
    "c5": (89040805632, 111620106752),
}
CNN_ROWS = [  # (name, group, offset, shape): the same in every configuration
    ("cnn.conv1.w", 0, 0, (64, 3, 3, 1)),
    ("cnn.conv1.b", 0, 576, (64,)),
    ("cnn.conv2.w", 0, 640, (128, 3, 3, 64)),
    ("cnn.conv2.b", 0, 74368, (128,)),
    ("cnn.conv3.w", 0, 74496, (256, 3, 3, 128)),
    ("cnn.conv3.b", 0, 369408, (256,)),
    ("cnn.bn3.w", 0, 369664, (256,)),
    ("cnn.bn3.b", 0, 369920, (256,)),
    ("cnn.conv4.w", 0, 370176, (256, 3, 3, 256)),
    ("cnn.conv4.b", 0, 960000, (256,)),
    ("cnn.conv5.w", 0, 960256, (512, 3, 3, 256)),
    ("cnn.conv5.b", 0, 2139904, (512,)),
    ("cnn.bn5.w", 0, 2140416, (512,)),
    ("cnn.bn5.b", 0, 2140928, (512,)),
    ("cnn.conv6.w", 0, 2141440, (512, 3, 3, 512)),
    ("cnn.conv6.b", 0, 4500736, (512,)),
    ("cnn.conv7.w", 0, 4501248, (512, 2, 2, 512)),
    ("cnn.conv7.b", 0, 5549824, (512,)),
    ("cnn.bn7.w", 0, 5550336, (512,)),
    ("cnn.bn7.b", 0, 5550848, (512,)),
]
TAIL_ROWS_HE256 = [  # c1 .. c4: one-layer BiLSTM(256), two-layer decoder
    ("enc_fw.l1.i2h.w", 1, 5551360, (1024, 512)),
    ("enc_fw.l1.i2h.b", 1, 6075648, (1024,)),
    ("enc_fw.l1.h2h.w", 1, 6076672, (1024, 256)),
    ("enc_fw.l1.h2h.b", 1, 6338816, (1024,)),
    ("enc_bw.l1.i2h.w", 2, 6339840, (1024, 512)),
    ("enc_bw.l1.i2h.b", 2, 6864128, (1024,)),
    ("enc_bw.l1.h2h.w", 2, 6865152, (1024, 256)),
    ("enc_bw.l1.h2h.b", 2, 7127296, (1024,)),
    ("dec.lookup", 3, 7128320, (39, 20)),
    ("dec.l1.i2h.w", 3, 7129100, (2048, 532)),
    ("dec.l1.i2h.b", 3, 8218636, (2048,)),
    ("dec.l1.h2h.w", 3, 8220684, (2048, 512)),
    ("dec.l1.h2h.b", 3, 9269260, (2048,)),
    ("dec.l2.i2h.w", 3, 9271308, (2048, 512)),
    ("dec.l2.i2h.b", 3, 10319884, (2048,)),
    ("dec.l2.h2h.w", 3, 10321932, (2048, 512)),
    ("dec.l2.h2h.b", 3, 11370508, (2048,)),
    ("dec.attn.wa", 3, 11372556, (512, 512)),
    ("dec.attn.wc", 3, 11634700, (512, 1024)),
    ("proj.w", 4, 12158988, (39, 512)),
    ("proj.b", 4, 12178956, (39,)),
]
TAIL_ROWS_C5 = [  # two-layer BiLSTM(512), two-layer decoder
    ("enc_fw.l1.i2h.w", 1, 5551360, (2048, 512)),
    ("enc_fw.l1.i2h.b", 1, 6599936, (2048,)),
    ("enc_fw.l1.h2h.w", 1, 6601984, (2048, 512)),
    ("enc_fw.l1.h2h.b", 1, 7650560, (2048,)),
    ("enc_fw.l2.i2h.w", 1, 7652608, (2048, 512)),
    ("enc_fw.l2.i2h.b", 1, 8701184, (2048,)),
    ("enc_fw.l2.h2h.w", 1, 8703232, (2048, 512)),
    ("enc_fw.l2.h2h.b", 1, 9751808, (2048,)),
    ("enc_bw.l1.i2h.w", 2, 9753856, (2048, 512)),
    ("enc_bw.l1.i2h.b", 2, 10802432, (2048,)),
    ("enc_bw.l1.h2h.w", 2, 10804480, (2048, 512)),
    ("enc_bw.l1.h2h.b", 2, 11853056, (2048,)),
    ("enc_bw.l2.i2h.w", 2, 11855104, (2048, 512)),
    ("enc_bw.l2.i2h.b", 2, 12903680, (2048,)),
    ("enc_bw.l2.h2h.w", 2, 12905728, (2048, 512)),
    ("enc_bw.l2.h2h.b", 2, 13954304, (2048,)),
    ("dec.lookup", 3, 13956352, (39, 20)),
    ("dec.l1.i2h.w", 3, 13957132, (4096, 1044)),
    ("dec.l1.i2h.b", 3, 18233356, (4096,)),
    ("dec.l1.h2h.w", 3, 18237452, (4096, 1024)),
    ("dec.l1.h2h.b", 3, 22431756, (4096,)),
    ("dec.l2.i2h.w", 3, 22435852, (4096, 1024)),
    ("dec.l2.i2h.b", 3, 26630156, (4096,)),
    ("dec.l2.h2h.w", 3, 26634252, (4096, 1024)),
    ("dec.l2.h2h.b", 3, 30828556, (4096,)),
    ("dec.attn.wa", 3, 30832652, (1024, 1024)),
    ("dec.attn.wc", 3, 31881228, (1024, 2048)),
    ("proj.w", 4, 33978380, (39, 1024)),
    ("proj.b", 4, 34018316, (39,)),
]
BUCKETS_HE256 = [(7128320, 12178995), (5551360, 7128320), (960256, 5551360), (0, 960256)]
BUCKETS_C5 = [(13956352, 34018355), (5551360, 13956352), (960256, 5551360), (0, 960256)]


@pytest.mark.parametrize("compute", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_layout_buckets_and_workspace(name, compute):
    import aocr
    B, H, W, He, Le, Ld, beam = CONFIGS[name]
    cfg = aocr.Config(B, H, W, He, Le, Ld, 39, 20, 1, 50, beam, compute)
    rows, counts = aocr.param_table(cfg)
    want = CNN_ROWS + (TAIL_ROWS_C5 if name == "c5" else TAIL_ROWS_HE256)
    assert rows == want
    assert sum(counts) == want[-1][2] + want[-1][3][0]                    # proj.b ends the flat vector
    b, e = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    assert aocr.lib.aocr_grad_buckets(C.byref(cfg), b, e) == 0
    assert list(zip(b, e)) == (BUCKETS_C5 if name == "c5" else BUCKETS_HE256)
    assert b[2] == dict((r[0], r[2]) for r in rows)["cnn.conv5.w"]       # the CNN group is split in front of conv5
    assert aocr.lib.aocr_workspace_bytes(C.byref(cfg)) == WORKSPACE[name][compute]


def test_bn_state_count():
    import aocr
    assert aocr.lib.aocr_bn_state_count() == 2560
