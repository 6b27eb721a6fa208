--[[ augment.lua -- host side of the on-device training augmentation (aocr_augment_lines and, before it, aocr_degrade_lines, include/aocr.h):
     the per-image records of a batch, drawn exactly as aocr/augment.py and aocr/degrade.py draw them (the composition is written out in Augmenter's docstring there), so that the
     Lua and the Python trainer draw the same records for the same (seed, counter), up to the last place of the platform's exp / sin /
     cos.  Used through DataGen:setAugment (lua/data_gen.lua).
     Needs LuaJIT 2.1: the bit.* functions on 64-bit cdata. ]]
local ffi = require 'ffi'
local bit = require 'bit'
require 'aocr_ffi'

local Augmenter = torch.class('Augmenter')
local U64 = ffi.typeof('uint64_t')

local function splitmix64(x)
    x = x + 0x9E3779B97F4A7C15ULL
    local z = bit.bxor(x, bit.rshift(x, 30)) * 0xBF58476D1CE4E5B9ULL
    z = bit.bxor(z, bit.rshift(z, 27)) * 0x94D049BB133111EBULL
    return bit.bxor(z, bit.rshift(z, 31))
end

-- opt: rotate_deg, shear, scale, translate = {x, y}, contrast, brightness, noise, fill, seed (defaults: no change, fill 255);
-- degrade: a Degrader (below) that DataGen runs before the warp, under the same counter, or nil
function Augmenter:__init(opt)
    opt = opt or {}
    self.degrade = opt.degrade
    self.rotate_deg, self.shear, self.scale = opt.rotate_deg or 0, opt.shear or 0, opt.scale or 1
    self.translate = opt.translate or {0, 0}
    self.contrast, self.brightness, self.noise = opt.contrast or 1, opt.brightness or 0, opt.noise or 0
    self.fill, self.seed = opt.fill or 255, opt.seed or 910820
end

-- aocr_warp[n] of batch `counter`: image i draws the uniforms 8 i .. 8 i + 7 of stream 0x41554700 + counter
function Augmenter:params(n, H, W, counter)
    local base = splitmix64(bit.bxor(U64(self.seed), U64(0x41554700 + counter) * 0xD1342543DE82EF95ULL))
    local warp = ffi.new('aocr_warp[?]', n)
    local cx, cy = (W - 1) / 2, (H - 1) / 2
    for i = 0, n - 1 do
        local j = {}
        for k = 0, 7 do
            local u = tonumber(bit.rshift(splitmix64(base + U64(8 * i + k)), 11)) * 2 ^ -53
            j[k] = 2 * u - 1
        end
        local theta, sh = math.rad(j[0] * self.rotate_deg), j[1] * self.shear
        local sx, sy = math.exp(j[2] * math.log(self.scale)), math.exp(j[3] * math.log(self.scale))
        local tx, ty = j[4] * self.translate[1], j[5] * self.translate[2]
        local g, b = math.exp(j[6] * math.log(self.contrast)), j[7] * self.brightness
        local cos, sin = math.cos(theta), math.sin(theta)
        local a00, a01 = cos / sx, (sh * cos - sin) / sy
        local a10, a11 = sin / sx, (sh * sin + cos) / sy
        local w = warp[i]                                                       -- + 0: -0 becomes +0, as on the Python side
        w.m00, w.m01, w.m02 = a00 + 0, a01 + 0, cx + tx - (a00 * cx + a01 * cy) + 0
        w.m10, w.m11, w.m12 = a10 + 0, a11 + 0, cy + ty - (a10 * cx + a11 * cy) + 0
        w.gain, w.offset, w.fill, w.noise = g, 128 * (1 - g) + b + 0, self.fill, self.noise
    end
    return warp
end

--[[ Degrader: the records of aocr_degrade_lines (elastic displacement, stroke weight, blur), as aocr/degrade.py composes them.
     opt: blur_sigma (0..1.5), thickness (-1..1), elastic = {x, y} (pixels, >= 0), pitch (integer >= 2), fill, seed; the defaults are the identity.
     The C call cannot check a record (it is device memory by then): the ranges are checked here. ]]
local Degrader = torch.class('Degrader')

function Degrader:__init(opt)
    opt = opt or {}
    self.blur_sigma, self.thickness, self.elastic = opt.blur_sigma or 0, opt.thickness or 0, opt.elastic or {0, 0}
    self.pitch, self.fill, self.seed = opt.pitch or 8, opt.fill or 255, opt.seed or 910820
    assert(self.blur_sigma >= 0 and self.blur_sigma <= 1.5, 'blur_sigma must be in 0..1.5: the blur has four taps a side, which would cut a wider Gaussian off visibly')
    assert(math.abs(self.thickness) <= 1, 'thickness must be in -1..1')
    assert(self.pitch >= 2 and self.pitch == math.floor(self.pitch), 'pitch must be an integer >= 2')
    assert(self.elastic[1] >= 0 and self.elastic[2] >= 0, 'elastic amplitudes are >= 0 pixels')
end

-- aocr_degrade[n] of batch `counter`: image i draws the uniforms 4 i .. 4 i + 3 of stream 0x4445475200000000 + counter
function Degrader:params(n, H, W, counter)
    local base = splitmix64(bit.bxor(U64(self.seed), (0x4445475200000000ULL + U64(counter)) * 0xD1342543DE82EF95ULL))
    local rec = ffi.new('aocr_degrade[?]', n)
    for i = 0, n - 1 do
        local u = {}
        for k = 0, 3 do u[k] = tonumber(bit.rshift(splitmix64(base + U64(4 * i + k)), 11)) * 2 ^ -53 end
        local sigma, r = u[0] * self.blur_sigma, rec[i]
        local w, sum = {[0] = 1, 0, 0, 0, 0}, 1
        if sigma > 0 then
            for k = 1, 4 do w[k] = math.exp(-(k * k) / (2 * sigma * sigma)); sum = sum + 2 * w[k] end
        end
        for k = 0, 4 do r.taps[k] = w[k] / sum end
        r.amp_x, r.amp_y = u[2] * self.elastic[1], u[3] * self.elastic[2]
        r.pitch, r.inv_pitch = self.pitch, 1 / self.pitch
        r.thick, r.fill = (2 * u[1] - 1) * self.thickness + 0, self.fill       -- + 0: -0 becomes +0, as on the Python side
    end
    return rec
end
