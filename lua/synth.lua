--[[ synth.lua -- host side of the on-device synthetic word lines (aocr_synth_lines, include/aocr.h): the per-image style records of a
     batch, drawn exactly as aocr/synth_lines.py draws them (the rule is written out in SynthGen's docstring there), so that the Lua and
     the Python trainer render the same crops for the same (seed, counter), up to the last place of the platform's exp / log.
     lexicon: {words = uint8_t[n_words * stride] (host copy), n_words =, stride =, desc = aocr_lexicon over the device copy};
     atlas:   {advance = uint8_t[n_faces * n_glyphs] (host copy), n_faces =, n_glyphs =, gh =, gw =, desc = aocr_glyph_atlas}.
     Needs LuaJIT 2.1: the bit.* functions on 64-bit cdata. ]]
local ffi = require 'ffi'
local bit = require 'bit'
local A = require 'aocr_ffi'

local SynthGen = torch.class('SynthGen')
local U64 = ffi.typeof('uint64_t')

local function splitmix64(x)
    x = x + 0x9E3779B97F4A7C15ULL
    local z = bit.bxor(x, bit.rshift(x, 30)) * 0xBF58476D1CE4E5B9ULL
    z = bit.bxor(z, bit.rshift(z, 27)) * 0x94D049BB133111EBULL
    return bit.bxor(z, bit.rshift(z, 31))
end

-- opt: width, seed, spacing = {lo, hi}, height = {lo, hi} (fractions of 32), stretch, fg = {lo, hi}, bg = {lo, hi}, fill_width
function SynthGen:__init(lexicon, atlas, opt)
    opt = opt or {}
    self.lexicon, self.atlas = lexicon, atlas
    self.width, self.seed = opt.width or 100, opt.seed or 910820
    self.spacing, self.height, self.stretch = opt.spacing or {0, 2}, opt.height or {0.6, 1.0}, opt.stretch or 1.25
    self.fg, self.bg = opt.fg or {0, 80}, opt.bg or {170, 255}
    self.fill_width = opt.fill_width ~= false
    self.synth_counter = 0                                                  -- +1 per batch; a resumed run sets it
end

-- the word's summed advance in `face` (0 for an id the atlas lacks) and its number of ids
local function measure(self, word, face)
    local lex, at = self.lexicon, self.atlas
    local sum, n = 0, 0
    for k = 0, lex.stride - 2 do
        local id = lex.words[word * lex.stride + k]
        if id == 0 then break end
        n = n + 1
        local g = id - 4
        if g >= 0 and g < at.n_glyphs then sum = sum + at.advance[face * at.n_glyphs + g] end
    end
    return sum, n
end

-- aocr_synth_style[n] of batch `counter`: image i draws the uniforms 9 i .. 9 i + 8 of stream 0x53594E00 + counter
function SynthGen:params(n, counter)
    local base = splitmix64(bit.bxor(U64(self.seed), U64(0x53594E00 + counter) * 0xD1342543DE82EF95ULL))
    local style = ffi.new('aocr_synth_style[?]', n)
    local W, H = self.width, 32
    local function r(u, range) return range[1] + u * (range[2] - range[1]) end
    for i = 0, n - 1 do
        local u = {}
        for k = 0, 8 do u[k] = tonumber(bit.rshift(splitmix64(base + U64(9 * i + k)), 11)) * 2 ^ -53 end
        local word = math.min(math.floor(u[0] * self.lexicon.n_words), self.lexicon.n_words - 1)
        local face = math.min(math.floor(u[1] * self.atlas.n_faces), self.atlas.n_faces - 1)
        local sp, th = r(u[2], self.spacing), H * r(u[3], self.height)
        local sy = self.atlas.gh / th
        local sum, ids = measure(self, word, face)
        local total = sum + math.max(ids - 1, 0) * sp
        local tw = W
        if not self.fill_width then tw = math.min(total / (sy * math.exp((2 * u[4] - 1) * math.log(self.stretch))), W) end
        local s = style[i]
        s.word, s.face, s.spacing, s.sy = word, face, sp, sy
        if total > 0 then s.sx, s.x0 = total / tw, u[5] * (W - tw) else s.sx, s.x0 = sy, u[5] * W end
        s.y0, s.fg, s.bg = u[6] * (H - th), r(u[7], self.fg), r(u[8], self.bg)
    end
    return style
end

-- one batch on the device: images (n,1,32,width) float, targets and targets_eval (n,L) int32 (device buffers of aocr_ffi), L = longest word + 1
function SynthGen:nextDevice(n)
    local style = self:params(n, self.synth_counter)
    self.synth_counter = self.synth_counter + 1
    local L = 1
    for i = 0, n - 1 do
        local _, ids = measure(self, style[i].word, style[i].face)
        L = math.max(L, ids + 1)
    end
    local bytes = n * ffi.sizeof('aocr_synth_style')
    local style_dev = A.device_bytes(bytes)
    A.upload(style_dev, style, bytes)
    local images, targets, targets_eval = A.device_bytes(n * 32 * self.width * 4), A.device_bytes(n * L * 4), A.device_bytes(n * L * 4)
    A.check(A.lib.aocr_synth_lines(nil, self.lexicon.desc, self.atlas.desc, style_dev:as('aocr_synth_style*'), n, 32, self.width, L,
                                   images:as('float*'), targets:as('int32_t*'), targets_eval:as('int32_t*')), 'aocr_synth_lines')
    style_dev:free()                                                        -- hipFree waits for the kernel that still reads it
    return images, targets, targets_eval, L
end
