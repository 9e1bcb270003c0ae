"use strict"
// Public surface of the Node host: what `import { SSGIEffect, TRAAEffect, VelocityDepthNormalPass } from "realism-effects"`
// gives for the hot path (src/index.js:1-31), plus the device (Renderer), the dump reader and checkpoint / resume of the temporal state (state.js).
module.exports = Object.assign({}, require("./effects"), require("./Renderer"), require("./dump"), require("./envmap"), require("./tiling"), require("./imageio"), require("./state"), require("./frames"))
