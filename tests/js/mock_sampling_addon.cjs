// mock_sampling_addon.cjs -- mock_addon.cjs plus the sampling entry points of lib/hgwarp.node, recorded in the same call log
// ("setSampling:<mode>", "multiSetSampling:<mode>").  TEST INFRASTRUCTURE ONLY (tests/js/sampling_class.mjs; HGWARP_ADDON=<this file>):
// it proves which addon calls the class makes for a sampling mode and in which order, not what the pixels are (the mock's warps are
// the nearest oracle's whatever the mode).
'use strict';
const base = require('./mock_addon.cjs');

const shim = Object.assign({}, base, {
    setSampling(c, mode) {
        if (mode !== 0 && mode !== 1) throw ('hgwarp mock: unknown sampling mode');
        base.calls.push(`setSampling:${mode}`); c.sampling = mode;
    },
    multiSetSampling(m, mode) {
        if (mode !== 0 && mode !== 1) throw ('hgwarp mock: unknown sampling mode');
        base.calls.push(`multiSetSampling:${mode}`); m.sampling = mode;
    },
});
module.exports = shim;
