"""numpy reference of aocr_lexicon_nearest (include/aocr.h) for the tests: the classic Levenshtein DP (string.levenshtein,
utils.lua:55-94, unit costs), vectorised over all words of a range -- one (n_words, m+1) array D[w][i] = distance of the first i
pattern ids to the first j ids of word w, advanced one word position j at a time -- then argmin, which returns the FIRST minimum:
lowest index on ties.  No bit vectors: nothing here shares an idea with the kernel."""
import numpy as np

EOS = 3


def cut(row):
    """the ids of a label row before its first EOS (what aocr_edit_distance compares)."""
    row = np.asarray(row).astype(np.int64)
    hit = np.nonzero(row == EOS)[0]
    return row[:hit[0]] if hit.size else row


def word_lengths(words_u8):
    """ids of every row of a (n, stride) uint8 word list before its first 0."""
    words_u8 = np.asarray(words_u8)
    return (np.cumsum(words_u8 == 0, axis=1) == 0).sum(axis=1)


def distances(pattern, words_u8):
    """Levenshtein distance of `pattern` (ids, any integers) to every word of words_u8 (n, stride) uint8."""
    pattern = np.asarray(pattern).astype(np.int64)
    words = np.asarray(words_u8).astype(np.int64)
    n, m = words.shape[0], pattern.shape[0]
    lens = word_lengths(words_u8)
    steps = np.arange(m + 1, dtype=np.int32)
    D = np.tile(steps, (n, 1))                                   # j = 0: i deletions
    out = np.full(n, -1, np.int64)
    out[lens == 0] = m
    for j in range(1, int(lens.max()) + 1 if n else 0):
        act = np.nonzero(lens >= j)[0]                           # words that still have an id at position j
        c = words[act, j - 1]
        prev = D[act]
        cur = np.empty_like(prev)
        cur[:, 0] = j
        cur[:, 1:] = np.minimum(prev[:, :-1] + (pattern[None, :] != c[:, None]), prev[:, 1:] + 1)      # substitute / match, skip the word's id
        cur = np.minimum.accumulate(cur - steps, axis=1) + steps                                       # skip pattern ids: cur[i] = min(cur[i], cur[i-1] + 1)
        D[act] = cur
        done = act[lens[act] == j]
        out[done] = D[done, m]
    return out


def nearest(labels, words_u8, row_begin=None):
    """(index, dist) int32 arrays: per row of labels (B, L), cut at its first EOS, the first word of its range at the smallest distance.
    row_begin (B+1) is clamped to [0, n_words]; an empty range gives -1 / -1; None searches the whole list."""
    labels = np.asarray(labels)
    words_u8 = np.asarray(words_u8)
    B, n = labels.shape[0], words_u8.shape[0]
    index, dist = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    rb = None if row_begin is None else np.clip(np.asarray(row_begin).astype(np.int64), 0, n)
    for b in range(B):
        lo, hi = (0, n) if rb is None else (int(rb[b]), int(rb[b + 1]))
        if hi <= lo:
            continue
        d = distances(cut(labels[b]), words_u8[lo:hi])
        k = int(np.argmin(d))
        index[b], dist[b] = lo + k, d[k]
    return index, dist
