// Homography.mjs -- drop-in `Homography` class for Node.js whose per-pixel work runs on an AMD MI355X (gfx950).
//
// Same public surface and state machine as Eric-Canas/Homography.js v1.8.0 (`import {Homography} from ...`):
//     new Homography(transform = 'auto', width = null, height = null)
//     setReferencePoints / setSourcePoints / setDestinyPoints / setImage / setTriangles / warp
//     getTransformationMatrixAsCSS
// Images are ImageData-shaped `{data: Uint8ClampedArray, width, height}` (what the reference accepts in Node, :297-299)
// and warp() returns the same shape.  The pixel loops, the triangle map and the per-triangle solves are NOT done in
// JavaScript: they go through the N-API addon lib/hgwarp.node -> C ABI libhgwarp.so -> HIP kernels.  There is no CPU
// fallback: without the addon or without a gfx950 GPU, construction throws.
//
// file:line comments cite the reference's Homography.js for the behaviour each method reproduces.  Reference quirks
// that are observable through the API are kept (SURVEY.md Appendix A), e.g. normalisation auto-detect (> 8.0), in-place
// (de)normalisation of caller-owned typed arrays, re-solving the inverse from swapped point sets.
//
// Differences, all Node-only consequences of having no DOM:
//   * HTMLImageElement inputs / asHTMLPromise / transformHTMLElement throw (the reference needs a browser for them too);
//   * (the reference's stale-state behaviour IS reproduced -- SURVEY.md Appendix A-Q12: one field holds the forward and the inverse
//     triangle map (:819-820 vs :847-848), so a forward piecewise warp that follows an inverse one indexes the stale INVERSE map
//     (:957); the per-triangle matrices survive setSourcePoints / setTriangles until the next setDestinyPoints (:252-255, :519,
//     :766).  The class mirrors both caches as value snapshots (`_map`, `_pm`) and hands the GPU exactly what the reference's loops
//     would read.  `new Homography(t, w, h, {repairStaleMap: true})` opts out: forward warps then always read the forward map of the
//     current mesh and every warp the matrices of the current point sets -- what the author evidently meant);
//   * frames of 1 MiB and more live in pooled page-locked memory handed out as external ArrayBuffers (no behavioural
//     difference; `Homography.release(imageData)` optionally returns a frame to the pool at once);
//   * Delaunator is not bundled: `Homography.triangulate` (default: ./delaunay.mjs, a restatement of delaunator 5's
//     sweep-hull algorithm that follows it step for step, so that triangle order and the diagonals of cocircular quads --
//     which decide pixels where triangles meet -- come out the same) supplies the triangles.  delaunator@5.0.0's source is
//     absent from the reference tree and none of its tests pins the triangulation, so identity with it is NOT claimed as
//     tested ("triangulation parity unpinned"); for guaranteed identical meshes pass delaunator's own output through
//     setTriangles() or assign Homography.triangulate.
import { createRequire } from 'module';
import { fileURLToPath } from 'url';
import path from 'path';
import { triangulate as defaultTriangulate } from './delaunay.mjs';

const require = createRequire(import.meta.url);
const HERE = path.dirname(fileURLToPath(import.meta.url));

let native = null;
function addon() {
    if (native === null) {
        const p = process.env.HGWARP_ADDON || path.join(HERE, '..', 'lib', 'hgwarp.node');
        try { native = require(p); } catch (e) {
            throw (`hgwarp: cannot load the native addon ${p} (${e && e.message ? e.message : e}); build it with \`make -C homography.js_amd\` -- there is no CPU fallback`);
        }
    }
    return native;
}

// When the page-locked frame pool starves (hgwarp_napi.c: poolPressure) a full collection would hand its dead frames back at
// once.  The library only ever asks for one when the USER started node with --expose-gc (global.gc exists); it never switches
// V8 flags itself and never forces collections on a host application that did not opt in -- without the flag, frames simply
// fall back to plain V8 arrays until V8 collects by itself (or the caller uses Homography.release(frame) / reuseOutput).
function collectGarbage() {
    if (typeof global.gc !== 'function') return false;
    global.gc();
    return true;
}
function makeRoomFor(native, bytes, n) {
    if (bytes >= 1048576 && native.poolPressure(bytes, n) && collectGarbage()) native.poolCollected();
}

const TRANSFORMS = ['auto', 'piecewiseaffine', 'affine', 'projective'];
const SAMPLING = ['nearest', 'bilinear'];       // index = HG_SAMPLE_NEAREST / HG_SAMPLE_BILINEAR
const CUBICS = { 'catmull-rom': [0, 0.5], 'mitchell': [1 / 3, 1 / 3], 'b-spline': [1, 0] };       // (B, C) of remap()'s named cubics
const CSS_DECIMALS = 5;                 // :31
const NORMALIZED_MAX = 8.0;             // :36  anything above is taken as pixel coordinates
const AFFINE = 0, PROJECTIVE = 1;

class WarpedImage {                     // ImageData-shaped result for runtimes without a global ImageData
    constructor(data, width, height) { this.data = data; this.width = width; this.height = height; }
}
const makeImageData = (data, w, h) => (typeof ImageData !== 'undefined' ? new ImageData(data, w, h) : new WarpedImage(data, w, h));

const anyAbove = (arr, limit) => { for (let i = 0; i < arr.length; i++) if (arr[i] > limit) return true; return false; };   // :1539
const toF32 = (points) => (ArrayBuffer.isView(points) ? points : new Float32Array(points.flat()));                          // :220 / :339
function scalePoints(p, sx, sy) { for (let i = 0; i < p.length; i++) p[i] = (i % 2) === 0 ? p[i] * sx : p[i] * sy; }       // :1603
function unscalePoints(p, sx, sy) { for (let i = 0; i < p.length; i++) p[i] = (i % 2) === 0 ? p[i] / sx : p[i] / sy; }     // :1621
// `new Uint8ClampedArray(n)` of the reference (:991, :1040) throws a RangeError for lengths V8 cannot allocate (Infinity from a
// degenerate matrix, > 2^31 - 1 under Node 12): same error here, before anything reaches the native side.
function checkedLength(n) { if (n > 2147483647) throw new RangeError(`Invalid typed array length: ${n}`); return n; }
const asF32 = (p) => (p instanceof Float32Array ? p : Float32Array.from(p));     // what the native side needs (values are already f32 when typed Float32Array)
// value equality of two point lists as the reference's Float32Array scratch triangles see them (:792-799); NaN equals NaN
function samePoints(a, b) {
    if (a.length !== b.length) return false;
    for (let i = 0; i < a.length; i++) { const x = Math.fround(a[i]), y = Math.fround(b[i]); if (x !== y && (x === x || y === y)) return false; }
    return true;
}
function sameTriangles(a, b) {
    if (a === b) return true;
    if (a === null || b === null || a.length !== b.length) return false;
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false;
    return true;
}
// `new Int16Array(n)` of the map builders (:820, :848): a negative length throws, NaN makes an empty array
function checkedMapLength(n) { if (n < 0 || n > 2147483647) throw new RangeError(`Invalid typed array length: ${n}`); return n; }

class Homography {
    constructor(transform = 'auto', width = null, height = null, options = {}) {
        if (width !== null) width = Math.round(width);          // :80-81
        if (height !== null) height = Math.round(height);
        this._width = width; this._height = height;
        this._objectiveWidth = null; this._objectiveHeight = null;
        this._xOutputOffset = undefined; this._yOutputOffset = undefined;
        this._srcPoints = null; this._dstPoints = null;
        this.firstTransformSelected = transform.toLowerCase();
        this.transform = transform.toLowerCase();
        this._image = null;
        this._maxSrcX = null; this._maxSrcY = null; this._minSrcX = null; this._minSrcY = null;
        this._srcPointsAreNormalized = true; this._dstPointsAreNormalized = true;
        // The two caches of the reference's piecewise path, mirrored as VALUE SNAPSHOTS of what they were computed from (the arrays
        // themselves live on the GPU and are rebuilt there):
        //   _map  <-> _trianglesCorrespondencesMatrix (:115): null | {kind: 'forward' | 'inverse', pts, tris, width, height, yOff} = the
        //             point set, triangles and geometry fillTriangle rasterised (:817-832 source points over the source bbox, :845-861
        //             destiny points over the output window).  Its null-ness steers re-triangulation (:252, :756); a forward warp reads
        //             WHATEVER it holds (:957);
        //   _pm   <-> _piecewiseMatrices (:119): null | {src, dst, tris} = the point sets and triangles the per-triangle matrices
        //             were solved from (:785-804); both warps use those matrices as they stand (:961, :1036-1038).
        this._map = null;
        this._pm = null;
        this._triangles = null;
        this._transformMatrix = null;
        // Opt-out of the stale-state quirks (header): forward warps always read the forward map of the current mesh, every warp the
        // matrices of the current point sets.
        this.repairStaleMap = options.repairStaleMap === true;
        this._lastPath = null;
        this._native = addon();                                 // throws if the addon is missing: there is no JS fallback
        this._device = options.device === undefined ? 0 : options.device;
        // Opt-in (not in the reference): warp() writes every frame of the inverse paths into one internal buffer and returns
        // a view of it, instead of allocating a fresh 4*w*h-byte array per call -- for frame loops that consume a frame
        // before asking for the next one.  Default false: a fresh array per call, like the reference (:991, :1040).
        this.reuseOutput = options.reuseOutput === true;
        this._outBuffer = null;
        // Opt-in (not in the reference), the same idea for warpBatch(): the frames of a batch are views of ONE page-locked buffer owned by
        // this instance and the NEXT warpBatch() on it overwrites them.  Default false: every frame owns its buffer, like the frames the
        // reference's loop returns -- `out.push(...h.warpBatch(chunk))` keeps working.  (Per call: warpBatch(sets, {reuseBatchOutput: true}).)
        this.reuseBatchOutput = options.reuseBatchOutput === true;
        // Opt-in (not in the reference): the caller promises not to mutate `image.data` between warps, so the source is
        // uploaded once per setImage() / context instead of on every warp().  Default false: the reference aliases the
        // caller's buffer and re-reads it on every warp (:298), so a mutated buffer must show up.
        this.staticImage = options.staticImage === true;
        this._uploadedImage = null;
        this._ctxHandle = null;                                 // GPU context, created at the first warp
        this._multiHandle = null; this._multiKey = null; this._multiImage = null;   // hg_multi over a device list (warpBatch({devices}))
        // Opt-in (not in the reference): {sampling: 'bilinear'} blends the four source pixels around each inverse-mapped coordinate
        // (include/hgwarp.h, hg_set_sampling) instead of copying the nearest one.  Every warp then takes the inverse loop -- the
        // forward (scatter) loops copy pixels by definition.  Default 'nearest': the reference's pixels, and no extra addon call.
        this._sampling = 'nearest';
        if (options.sampling !== undefined) this.sampling = options.sampling;
    }

    /** 'nearest' (default, the reference's pixel copy) or 'bilinear' (opt-in); applies to the warps called from now on. */
    get sampling() { return this._sampling; }
    set sampling(mode) {
        if (!SAMPLING.includes(mode)) throw (`hgwarp: sampling must be 'nearest' or 'bilinear', but ${mode} was given`);
        if (mode === this._sampling) return;
        this._sampling = mode;
        if (this._ctxHandle) this._native.setSampling(this._ctxHandle, SAMPLING.indexOf(mode));
        if (this._multiHandle) this._native.multiSetSampling(this._multiHandle, SAMPLING.indexOf(mode));
    }

    /** Which map the shared field would hold: null | 'forward' | 'inverse'. */
    get _mapState() { return this._map === null ? null : this._map.kind; }

    /** GPU context of this instance (one hg_ctx per Homography).  Throws a string without a usable gfx950 device. */
    get _ctx() {
        if (this._ctxHandle === null) {
            this._ctxHandle = this._native.create(this._device);
            if (this._sampling !== 'nearest') this._native.setSampling(this._ctxHandle, SAMPLING.indexOf(this._sampling));
        }
        return this._ctxHandle;
    }

    /** Frees the GPU context (optional; it is also released when the object is garbage-collected). */
    close() {
        if (this._ctxHandle) { this._native.destroy(this._ctxHandle); this._ctxHandle = null; }
        if (this._multiHandle) { this._native.multiDestroy(this._multiHandle); this._multiHandle = null; this._multiKey = null; }
    }

    // ------------------------------------------------------------------------------------------------ public setters
    setReferencePoints(srcPoints, dstPoints, image = null, width = null, height = null, srcPointsAreNormalized = null, dstPointsAreNormalized = null) {   // :173-182
        if (typeof (srcPoints) === 'undefined' || typeof (dstPoints) === 'undefined') {
            throw ("Source and Destiny points must be defined when calling setReferencePoints().");
        }
        this._dstPoints = null;
        this.setSourcePoints(srcPoints, image, width, height, srcPointsAreNormalized);
        this.setDestinyPoints(dstPoints, dstPointsAreNormalized);
    }

    setSourcePoints(points, image = null, width = null, height = null, pointsAreNormalized = null) {    // :218-265
        points = toF32(points);
        this._srcPoints = points;
        this._srcPointsAreNormalized = pointsAreNormalized === null ? !anyAbove(points, NORMALIZED_MAX) : pointsAreNormalized;
        this._transformMatrix = null;
        this.transform = selectTransform(this.firstTransformSelected, points);
        this._objectiveWidth = null; this._objectiveHeight = null;
        if (image !== null) this.setImage(image, width, height);
        else if (width !== null || height !== null) this._setSourceSize(width, height);
        if (this._width !== null && this._height !== null && this._srcPointsAreNormalized) {
            scalePoints(this._srcPoints, this._width, this._height);
            this._srcPointsAreNormalized = false;
        }
        if (this._dstPoints !== null && this.transform !== 'piecewiseaffine') {
            this._transformMatrix = this._solve(this._srcPoints, this._dstPoints);
        }
        if (this.transform === 'piecewiseaffine' && this._map === null) {
            this._triangles = null;                             // :254 (_initialTriangles is never set by the reference)
            this._pm = null;                                    // :255 (ONLY here: with a map in place the old matrices survive new source points)
            if (!this._srcPointsAreNormalized || (this._width > 0 && this._height > 0)) this._refreshPiecewise();
            else if (this._triangles === null) this._triangles = Homography.triangulate(this._srcPoints);
        }
    }

    setImage(image, width = null, height = null) {                                                      // :290-316
        if (!image || !ArrayBuffer.isView(image.data)) {
            throw ("hgwarp: setImage() needs an ImageData-shaped {data: Uint8ClampedArray, width, height}; HTMLImageElement inputs need a browser DOM");
        }
        this._image = image.data;                               // aliased, not copied (:298): re-read (re-uploaded) on every warp()
        this._uploadedImage = null;                             // (staticImage: an explicit setImage always uploads)
        this._setSourceSize(image.width, image.height);
        if (this._srcPoints !== null && this.transform === 'piecewiseaffine') this._refreshPiecewise();
        if (this._dstPoints !== null && (this._objectiveWidth <= 0 || this._objectiveHeight <= 0)) this._deriveOutputWindow();
    }

    setDestinyPoints(points, pointsAreNormalized = null) {                                              // :337-380
        points = toF32(points);
        if (this._srcPoints !== null && points.length !== this._srcPoints.length) {
            throw (`It must be the same amount of destiny points (${points.length / 2}) than source points (${this._srcPoints.length / 2})`);
        }
        this._dstPoints = points;
        this._dstPointsAreNormalized = pointsAreNormalized === null ? !anyAbove(points, NORMALIZED_MAX) : pointsAreNormalized;
        if (this.transform !== 'piecewiseaffine') {
            if (this._dstPointsAreNormalized && this._width > 0 && this._height > 0 && this.transform === 'projective') {
                scalePoints(this._dstPoints, this._width, this._height);
                this._dstPointsAreNormalized = false;
            }
            this._alignRanges();
            this._transformMatrix = this._solve(this._srcPoints, this._dstPoints);
        } else {
            this._pm = null;                                    // :361
        }
        if (this._image !== null || (this.transform === 'piecewiseaffine' && this._width > 0 && this._height > 0)) this._deriveOutputWindow();
        if (this.transform === 'piecewiseaffine' && this._width > 0 && this._height > 0) {
            if (this._dstPointsAreNormalized) { scalePoints(this._dstPoints, this._width, this._height); this._dstPointsAreNormalized = false; }
            this._refreshPiecewise();
        }
    }

    setTriangles(triangles) {                                                                           // :517-524
        this._triangles = triangles;
        if ((!this._srcPointsAreNormalized || (this._width > 0 && this._height > 0)) && this._srcPoints !== null) this._refreshPiecewise();
    }

    // ------------------------------------------------------------------------------------------------ warp
    warp(image = null, asHTMLPromise = false, applyAlwaysInverse = false) {                             // :408-446
        if (image !== null) this.setImage(image);
        else if (this._image === null) {
            throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");
        }
        if (asHTMLPromise) throw ("hgwarp: asHTMLPromise needs a browser DOM; use the returned ImageData-shaped object");
        const forward = this._dispatchesForward(applyAlwaysInverse);
        let out;
        switch (this.transform) {
            case 'piecewiseaffine':
                out = forward ? this._forwardPiecewise() : this._inversePiecewise();
                break;
            case 'affine':
                out = forward ? this._forwardGeometric() : this._inverseGeometric();
                break;
            case 'projective':
                out = this._inverseGeometric();
                break;
        }
        const area = this._objectiveWidth * this._objectiveHeight;
        if (area >= 1 && !isNaN(area)) return makeImageData(out, this._objectiveWidth, this._objectiveHeight);
        return makeImageData(new Uint8ClampedArray(4), 1, 1);                                           // :440
    }

    /** Does warp(null, false, applyAlwaysInverse) take a forward (scatter) loop for the current state?  (:421-422, :426-427, :431; bilinear
     *  sampling always takes the inverse loop: the forward loops have nothing to blend.) */
    _dispatchesForward(applyAlwaysInverse = false) {
        if (applyAlwaysInverse || this._sampling === 'bilinear') return false;
        if (this.transform === 'piecewiseaffine')
            return !(this._objectiveWidth > this._width || this._objectiveHeight > this._height ||
                     this._objectiveWidth * 1.2 < this._width || this._objectiveHeight * 1.2 < this._height);
        if (this.transform === 'affine') return !(this._objectiveWidth !== this._width || this._objectiveHeight !== this._height);
        return false;
    }

    /**
     * The SOURCE FIELD of the inverse loop for the instance's current transform and points, over the window warp() would use (not part of
     * the reference; include/hgwarp.h, HG_FIELD_*): for every output pixel, which source pixel `warp(null, false, true)` copies.
     *   'index'   Int32Array, one flat pixel index per output pixel, -1 where the loop writes nothing or reads outside the array:
     *             out32[i] = data[i] >= 0 ? image32[data[i]] : 0 is warp(null, false, true).data, byte for byte;
     *   'coords'  Float32Array, (sx, sy) per output pixel (the loop's f64 coordinate rounded once), NaN where the loop's test fails.
     * options.loop picks the loop whose field this is:
     *   'inverse' (default)  always the inverse loop, whatever warp() would dispatch to;
     *   'warp'               the loop warp() would dispatch to for the current state (the same tests as warp(), bilinear sampling -> inverse
     *                        included): gathered over the image, `data` IS warp().data -- for a same-size piecewise or affine frame that
     *                        is the forward (scatter) loop, holes, overwritten pixels and aliased columns included;
     *   'forward'            always the forward loop (_piecewiseAffineWarp / _geometricWarp with the forward matrix).
     * A forward field is 'index' only (the forward loops copy whole pixels from integer positions: (i % width, i / width) of the source is
     * the coordinate): data[p] is the flat source index the LAST writer of output pixel p reads, -1 where nobody writes or that read lies
     * outside the image.  The reference-state forms of the forward loop (a stale map or stale matrices, as warp() would replay them) have
     * no field.
     * Independent of the sampling mode otherwise; records neither a map nor a path (the reference-visible state stays that of the last
     * warp).  Masks, depth maps, labels go through the picture's geometry by a gather over `data`.
     * Returns { data, width, height }.  Throws a string for an unknown format or loop, for 'coords' with a forward loop, and for the
     * reference-state quirks unless `repairStaleMap` is set (matrices of an older point set after setSourcePoints / setTriangles without a
     * setDestinyPoints; for a forward piecewise loop also a map field that does not hold the forward map of the current mesh, e.g. after an
     * inverse warp): call setDestinyPoints / setSourcePoints first.
     */
    sourceField(format = 'index', options = {}) {
        if (format !== 'index' && format !== 'coords') throw ("sourceField: format must be 'index' or 'coords'");
        const fmt = format === 'index' ? 0 : 1;
        const call = this._fieldCall('sourceField', fmt, options);
        if (call === null) return { data: fmt === 0 ? new Int32Array(0) : new Float32Array(0), width: 0, height: 0 };
        return { data: this._native['field' + call.entry](this._ctx, ...call.args), width: call.width, height: call.height };
    }

    /**
     * One plane that lies beside the picture -- a mask, labels, depth, float features, a second picture -- through the geometry
     * sourceField() would export for the current state, ON THE DEVICE (not part of the reference): the field is computed into device
     * memory and never comes to the host; the plane goes up, the library's remap runs, the result comes down.
     *   plane             a typed array of width * height * channels elements over the instance's image size;
     *   options.channels  interleaved channels per pixel (default 1);
     *   options.sampling  'nearest' (default): through the 'index' field; pixels are opaque blocks of channels * BYTES_PER_ELEMENT bytes
     *                     (1, 2, 4, 8 or 16), any typed array class -- remap(new Uint32Array(image.data.buffer)) IS warp(null, false, true);
     *                     'bilinear': through the 'coords' field; a Float32Array, Uint8Array or Uint8ClampedArray of 1..4 channels, blended
     *                     in f32 in the operation order of the bilinear sampling mode; bytes are rounded min(255, floor(v + 0.5)), 4 channels
     *                     being straight (not premultiplied) RGBA; an uncovered pixel is 0 in every channel;
     *                     'trilinear': 'bilinear' with minification filtering -- the same planes, field and refusals; the plane's mip
     *                     pyramid (all levels) is built in device scratch and every pixel blends the two levels that match the field's
     *                     own footprint there (include/hgwarp.h, hg_remap_trilinear_frames_device), so a shrink no longer aliases; where
     *                     the field does not shrink the result is 'bilinear''s, bit for bit;
     *                     'anisotropic': 'trilinear' for oblique views -- up to options.maxAniso probes along the longer of a pixel's two
     *                     steps in the field, each from the finer level(s) the shorter step allows, averaged (include/hgwarp.h,
     *                     hg_remap_aniso_frames_device), so the axis that shrinks less stays sharp; maxAniso 1 is 'trilinear', bit for bit;
     *                     'bicubic': 'bilinear' for ENLARGEMENTS -- the same planes, field and refusals; 4 x 4 taps weighted by the cubic
     *                     options.cubic names (include/hgwarp.h, hg_remap_bicubic_frames_device), so edges and curves survive a 3-4x
     *                     magnification; bytes are clamped to 0..255 on both sides (the cubic overshoots beside an edge); it reads the
     *                     plane itself only, so a shrink aliases as 'bilinear' does -- 'trilinear' / 'anisotropic' are for shrinking;
     *   options.maxAniso  'anisotropic' only: an integer in 1..16 (default 8), the most probes a pixel takes;
     *   options.cubic     'bicubic' only: 'catmull-rom' (default; interpolates: integer coordinates give the source pixel), 'mitchell',
     *                     'b-spline' (smoothest, never overshoots), or [B, C] with two finite numbers in [0, 1];
     *   options.loop      'inverse' (default), 'warp' or 'forward': sourceField's meaning, refusals and stale-state rules; 'bilinear',
     *                     'bicubic', 'trilinear' and 'anisotropic' with a forward loop throw, as 'coords' does there.
     * Independent of the instance's sampling mode; records neither a map nor a path.
     * Returns { data, width, height, channels }, `data` being of the plane's own class; an empty window gives empty data, width and height 0.
     */
    remap(plane, options = {}) {
        if (options === null || options === undefined) options = {};
        const sampling = options.sampling === undefined ? 'nearest' : options.sampling;
        if (sampling !== 'nearest' && sampling !== 'bilinear' && sampling !== 'bicubic' && sampling !== 'trilinear' && sampling !== 'anisotropic')
            throw ("remap: options.sampling must be 'nearest', 'bilinear', 'bicubic', 'trilinear' or 'anisotropic'");
        const maxAniso = options.maxAniso === undefined ? 8 : options.maxAniso;
        if (sampling === 'anisotropic' && !(Number.isInteger(maxAniso) && maxAniso >= 1 && maxAniso <= 16)) throw ("remap: options.maxAniso must be an integer in 1..16");
        let cubic = CUBICS['catmull-rom'];
        if (sampling === 'bicubic' && options.cubic !== undefined) {
            cubic = typeof options.cubic === 'string' && Object.prototype.hasOwnProperty.call(CUBICS, options.cubic) ? CUBICS[options.cubic] : options.cubic;
            if (!(Array.isArray(cubic) && cubic.length === 2 && cubic.every((v) => typeof v === 'number' && v >= 0 && v <= 1)))
                throw ("remap: options.cubic must be 'catmull-rom', 'mitchell', 'b-spline' or [B, C] with two numbers in [0, 1]");
        }
        const channels = options.channels === undefined ? 1 : options.channels;
        if (!ArrayBuffer.isView(plane) || plane instanceof DataView) throw ("remap: plane must be a typed array");
        if (!Number.isInteger(channels) || channels < 1) throw ("remap: options.channels must be a positive integer");
        if (sampling !== 'nearest') {
            if (!(plane instanceof Float32Array || plane instanceof Uint8Array || plane instanceof Uint8ClampedArray))
                throw (`remap: a '${sampling}' plane must be a Float32Array, Uint8Array or Uint8ClampedArray`);
            if (channels > 4) throw (`remap: a '${sampling}' plane has 1 to 4 channels`);
        } else if (![1, 2, 4, 8, 16].includes(channels * plane.BYTES_PER_ELEMENT)) {
            throw ("remap: a 'nearest' pixel (channels * BYTES_PER_ELEMENT) must be 1, 2, 4, 8 or 16 bytes");
        }
        const fmt = sampling === 'nearest' ? 0 : 1;
        const call = this._fieldCall('remap', fmt, options);          // (throws without an image)
        if (plane.length !== this._width * this._height * channels) throw ("remap: plane must hold width * height * channels elements of the instance's image size");
        if (call === null) return { data: new plane.constructor(0), width: 0, height: 0, channels };
        const data = sampling === 'anisotropic'
            ? this._native['remapAniso' + call.entry](this._ctx, ...call.args, plane, channels, this._width, this._height, maxAniso)
            : sampling === 'bicubic'
            ? this._native['remapBicubic' + call.entry](this._ctx, ...call.args, plane, channels, this._width, this._height, cubic[0], cubic[1])
            : this._native[(sampling === 'trilinear' ? 'remapTrilinear' : 'remap') + call.entry](this._ctx, ...call.args, plane, channels, this._width, this._height);
        return { data, width: call.width, height: call.height, channels };
    }

    /**
     * A list of points through the geometry sourceField() would export for the current state, on the device (not part of the reference):
     * landmarks, box corners, contour vertices, a click position.
     *   points       a Float32Array or an array of x,y pairs, in pixels;
     *   options.to   'output' (default): source-image positions -> positions in the output window (the forward loop: the value it hands to
     *                Math.round, window-relative, reported whether or not it falls inside the window); a point maps iff its cell
     *                (Math.round of each coordinate) lies in the forward loop's domain -- the image for affine / projective, a covered cell
     *                of the source mesh for piecewise;
     *                'source': positions in the output window (output pixel (i, j) is the point (i, j)) -> source coordinates (the inverse
     *                loop); a point maps iff its cell lies in the window and its coordinate passes the loop's coverage test -- for integer
     *                positions the value of sourceField('coords') at that pixel, bit for bit.
     * Refusals, stale-state rules (`repairStaleMap`), solves and uploads are sourceField's for loop 'forward' resp. 'inverse'.  Records
     * neither a map nor a path.  Returns a Float32Array of the same length, NaN in both coordinates of an unmapped point; an empty window
     * gives all NaN.  Throws a string for an unknown `to` or a list that does not hold pairs.
     */
    transformPoints(points, options = {}) {
        if (options === null || options === undefined) options = {};
        const to = options.to === undefined ? 'output' : options.to;
        if (to !== 'output' && to !== 'source') throw ("transformPoints: options.to must be 'output' or 'source'");
        if (!(points instanceof Float32Array) && !Array.isArray(points)) throw ("transformPoints: points must be a Float32Array or an array of x,y pairs");
        const pts = points instanceof Float32Array ? points : Float32Array.from(points.flat());
        if (pts.length % 2 !== 0) throw ("transformPoints: points must hold x,y pairs");
        const call = this._fieldCall('transformPoints', to === 'output' ? 0 : 1, { loop: to === 'output' ? 'forward' : 'inverse' });
        if (call === null || pts.length === 0) return new Float32Array(pts.length).fill(NaN);
        return this._native['points' + call.entry](this._ctx, ...call.args, pts);
    }

    /**
     * One transform per frame from point MATCHES, robust to wrong ones (not part of the reference; hg_fit_matches_frames_device in
     * include/hgwarp.h has the rules): RANSAC over `hypotheses` minimal samples per frame, the best one refitted by least squares over its
     * inliers.  matchSets: an array of F lists, each a Float32Array of x, y, u, v quadruples or an array of [x, y, u, v]; (x, y) is the FROM
     * position, (u, v) the TO position and the matrix maps from -> to.  The lengths may differ: the lists are padded to the longest and the
     * device is told each frame's count.
     * options: { transform: 'projective' (default) | 'affine', threshold = 3 (pixels), hypotheses = 1024 (0: plain least squares over every
     *            finite match; needs refit), seed = 0, refit = true, samples: Int32Array of F x hypotheses x 4 indices instead of drawn ones }.
     * Returns { kind, matrices: Float64Array(8 F) -- the result to use, row f at 8 f; affine in the first 6 of each 8; NaN for a frame
     *           without a valid hypothesis --, minimal: Float64Array(8 F) -- the best hypothesis' matrix as solved --, counts: Int32Array(F),
     *           best: Int32Array(F) (-1: failed), inliers: [Uint8Array(n_f), ...] one flag per match of frame f }.
     * `matrices` go straight into the geometric batch calls; calculateTransformLimits-style windows come from hg_transform_limits.
     * Needs no image and changes no state of the instance.  Throws a bare string for an unknown transform, a list whose length is not a
     * multiple of 4, a bad threshold or a bad hypotheses count.
     */
    fitMatches(matchSets, options = {}) {
        if (options === null || options === undefined) options = {};
        const transform = options.transform === undefined ? 'projective' : options.transform;
        if (transform !== 'projective' && transform !== 'affine') throw ("fitMatches: options.transform must be 'projective' or 'affine'");
        if (!Array.isArray(matchSets)) throw ("fitMatches: matchSets must be an array of match lists");
        if (matchSets.length > 4096) throw ("fitMatches: at most 4096 frames");
        const threshold = options.threshold === undefined ? 3 : options.threshold;
        if (typeof threshold !== 'number' || !Number.isFinite(threshold) || threshold < 0) throw ("fitMatches: options.threshold must be a finite number >= 0");
        const hypotheses = options.hypotheses === undefined ? 1024 : options.hypotheses;
        if (!Number.isInteger(hypotheses) || hypotheses < 0 || hypotheses > 65536) throw ("fitMatches: options.hypotheses must be an integer in 0..65536");
        const refit = options.refit === undefined ? true : !!options.refit;
        if (hypotheses === 0 && !refit) throw ("fitMatches: options.hypotheses = 0 is the least-squares fit and needs refit");
        const seed = options.seed === undefined ? 0 : options.seed;
        if (!Number.isInteger(seed) || seed < 0 || seed > 0xffffffff) throw ("fitMatches: options.seed must be an integer in 0..2^32-1");
        const lists = matchSets.map((s, f) => {
            if (!(s instanceof Float32Array) && !Array.isArray(s)) throw ("fitMatches: match list " + f + " must be a Float32Array or an array of [x, y, u, v]");
            const l = s instanceof Float32Array ? s : Float32Array.from(s.flat());
            if (l.length % 4 !== 0) throw ("fitMatches: match list " + f + " must hold x, y, u, v quadruples");
            return l;
        });
        const F = lists.length, nPoints = lists.reduce((m, l) => Math.max(m, l.length / 4), 0);
        if (nPoints > 65536) throw ("fitMatches: at most 65536 matches per frame");
        const counts = Int32Array.from(lists, (l) => l.length / 4);
        const packed = new Float32Array(F * nPoints * 4);
        lists.forEach((l, f) => packed.set(l, f * nPoints * 4));
        let samples = null;
        if (options.samples !== undefined && options.samples !== null) {
            samples = options.samples instanceof Int32Array ? options.samples : Int32Array.from(options.samples.flat(Infinity));
            if (samples.length !== F * hypotheses * 4) throw ("fitMatches: options.samples must hold frames x hypotheses x 4 indices");
        }
        const r = this._native.fitMatches(this._ctx, transform === 'projective' ? 1 : 0, packed, nPoints, counts, threshold, hypotheses, seed, samples, refit ? 1 : 0);
        const inliers = lists.map((l, f) => r.mask.slice(f * nPoints, f * nPoints + counts[f]));
        return { kind: transform, matrices: r.matrices, minimal: r.minimal, counts: r.counts, best: r.best, inliers };
    }

    /**
     * The frame -> canvas matrices of a frame set adjusted over ALL pairs at once (not part of the reference; hg_bundle_adjust_frames_device
     * in include/hgwarp.h has the rules): Levenberg-Marquardt on the disagreement, in the canvas, of the matches of every pair.  The
     * planar-mosaic formulation: at least one frame is held fixed, the unknowns are the entries of the matrices; no camera model, no lens
     * terms.  A local refinement: start from chainMatrices().
     * matrices: Float64Array(8 F) or an array of 8 F numbers, frame -> canvas; pairs: an array of [a, b] (or an Int32Array of 2 P indices);
     * matchSets: one list per pair, a Float32Array of x, y, u, v quadruples or an array of [x, y, u, v] -- (x, y) in frame a, (u, v) in frame
     * b; the lists are padded to the longest and the device is told each pair's count.
     * options: { transform: 'projective' (default) | 'affine', width, height (of every frame), fixed = [0] (frame indices), iterations = 10,
     *            eps = 0.01 (canvas pixels), lambda = 1e-3 (the first damping), huber = 0 (pixels; 0: off), masks: one Uint8Array per pair
     *            (0 = leave the match out; what fitMatches() returns as `inliers`) }.
     * Returns { matrices: Float64Array(8 F), status (0 converged, 1 ran all iterations, 2 stalled, 3 singular), rounds, accepted, rmsFirst,
     *           rmsLast (canvas pixels), frames: Int32Array(F) (0 adjusted, 1 fixed, 2 unanchored, 3 bad input), pairs: [{ nValidFirst,
     *           nValidLast, rmsFirst, rmsLast }, ...] -- which names the pair that does not fit }.
     * Needs no image and changes no state of the instance.  Throws a bare string for a bad option, pair or list.
     */
    bundleAdjust(matrices, pairs, matchSets, options = {}) {
        if (options === null || options === undefined) options = {};
        const transform = options.transform === undefined ? 'projective' : options.transform;
        if (transform !== 'projective' && transform !== 'affine') throw ("bundleAdjust: options.transform must be 'projective' or 'affine'");
        const isInt = (v, lo, hi) => Number.isInteger(v) && v >= lo && v <= hi;
        const { width, height } = options;
        if (!isInt(width, 1, 32768) || !isInt(height, 1, 32768)) throw ("bundleAdjust: options.width and options.height must be integers in 1..32768");
        const iterations = options.iterations === undefined ? 10 : options.iterations;
        if (!isInt(iterations, 0, 64)) throw ("bundleAdjust: options.iterations must be an integer in 0..64");
        const num = (v, d) => (v === undefined ? d : v);
        const eps = num(options.eps, 0.01), lambda = num(options.lambda, 1e-3), huber = num(options.huber, 0);
        if (typeof eps !== 'number' || !Number.isFinite(eps) || eps < 0) throw ("bundleAdjust: options.eps must be a finite number >= 0");
        if (typeof lambda !== 'number' || !Number.isFinite(lambda) || lambda <= 0) throw ("bundleAdjust: options.lambda must be a finite number > 0");
        if (typeof huber !== 'number' || !Number.isFinite(huber) || huber < 0) throw ("bundleAdjust: options.huber must be a finite number >= 0");
        if (!(matrices instanceof Float64Array) && !Array.isArray(matrices)) throw ("bundleAdjust: matrices must be a Float64Array or an array of numbers");
        const mats = matrices instanceof Float64Array ? matrices : Float64Array.from(matrices.flat());
        if (mats.length % 8 !== 0) throw ("bundleAdjust: matrices must hold 8 numbers per frame");
        const F = mats.length / 8;
        if (F > 256) throw ("bundleAdjust: at most 256 frames");
        const P2 = this._bundlePairs('bundleAdjust', pairs, F);
        const P = P2.length / 2;
        if (!Array.isArray(matchSets) || matchSets.length !== P) throw ("bundleAdjust: matchSets must be an array of one match list per pair");
        const fixedList = options.fixed === undefined ? (F > 0 ? [0] : []) : options.fixed;
        if (!Array.isArray(fixedList) || !fixedList.every((f) => isInt(f, 0, F - 1))) throw ("bundleAdjust: options.fixed must be an array of frame indices");
        if (F > 0 && fixedList.length === 0) throw ("bundleAdjust: options.fixed must name at least one frame");
        const fixed = new Uint8Array(F);
        fixedList.forEach((f) => { fixed[f] = 1; });
        const lists = matchSets.map((s, p) => {
            if (!(s instanceof Float32Array) && !Array.isArray(s)) throw ("bundleAdjust: match list " + p + " must be a Float32Array or an array of [x, y, u, v]");
            const l = s instanceof Float32Array ? s : Float32Array.from(s.flat());
            if (l.length % 4 !== 0) throw ("bundleAdjust: match list " + p + " must hold x, y, u, v quadruples");
            return l;
        });
        const nPoints = lists.reduce((m, l) => Math.max(m, l.length / 4), 0);
        if (nPoints > 65536) throw ("bundleAdjust: at most 65536 matches per pair");
        const counts = Int32Array.from(lists, (l) => l.length / 4);
        const packed = new Float32Array(P * nPoints * 4);
        lists.forEach((l, p) => packed.set(l, p * nPoints * 4));
        let mask = null;
        if (options.masks !== undefined && options.masks !== null) {
            if (!Array.isArray(options.masks) || options.masks.length !== P) throw ("bundleAdjust: options.masks must be an array of one mask per pair");
            mask = new Uint8Array(P * nPoints);
            options.masks.forEach((k, p) => {
                if ((!(k instanceof Uint8Array) && !Array.isArray(k)) || k.length !== counts[p]) throw ("bundleAdjust: mask " + p + " must hold one flag per match of its pair");
                mask.set(k, p * nPoints);
            });
        }
        const r = this._native.bundleAdjust(this._ctx, transform === 'projective' ? 1 : 0, width, height, fixed, P2, packed, nPoints, counts, mask, iterations, eps, lambda,
                                            huber, mats);
        if (F === 0) return { matrices: r.matrices, status: 1, rounds: 0, accepted: 0, rmsFirst: NaN, rmsLast: NaN, frames: new Int32Array(0), pairs: [] };
        const v = new DataView(r.info.buffer, r.info.byteOffset, r.info.byteLength);
        const frames = Int32Array.from({ length: F }, (_, f) => v.getInt32(48 + 4 * f, true));
        const o = 48 + ((4 * F + 7) & ~7);
        const perPair = Array.from({ length: P }, (_, p) => ({ nValidFirst: v.getInt32(o + 24 * p, true), nValidLast: v.getInt32(o + 24 * p + 4, true),
                                                                rmsFirst: v.getFloat64(o + 24 * p + 8, true), rmsLast: v.getFloat64(o + 24 * p + 16, true) }));
        return { matrices: r.matrices, status: v.getInt32(0, true), rounds: v.getInt32(4, true), accepted: v.getInt32(8, true), rmsFirst: v.getFloat64(24, true),
                 rmsLast: v.getFloat64(32, true), frames, pairs: perPair };
    }

    _bundlePairs(who, pairs, F) {
        if (!(pairs instanceof Int32Array) && !Array.isArray(pairs)) throw (who + ": pairs must be an array of [a, b] or an Int32Array");
        const flat = pairs instanceof Int32Array ? pairs : pairs.flat();
        if (flat.length % 2 !== 0) throw (who + ": pairs must hold two frame indices each");
        if (flat.length / 2 > 8192) throw (who + ": at most 8192 pairs");
        for (let p = 0; p < flat.length; p += 2) {
            const a = flat[p], b = flat[p + 1];
            if (!Number.isInteger(a) || !Number.isInteger(b) || a < 0 || b < 0 || a >= F || b >= F || a === b) throw (who + ": pair " + (p / 2) + " must name two different frames");
        }
        return pairs instanceof Int32Array ? pairs : Int32Array.from(flat);
    }

    /**
     * Frame -> canvas matrices chained from pairwise ones, the start bundleAdjust() wants (hg_bundle_chain_from_pairs; host only).
     * pairMatrices: Float64Array(8 P) or an array of 8 P numbers, matrix p maps frame a to frame b of pairs[p] -- what fitMatches() returns
     * with a as FROM; options: { frames (required), anchor = 0, transform: 'projective' (default) | 'affine' }.  The anchor is the identity,
     * frames are reached breadth-first, pairs whose matrix is not finite are skipped, frames never reached come back as NaNs.
     * Returns Float64Array(8 frames).
     */
    chainMatrices(pairMatrices, pairs, options = {}) {
        if (options === null || options === undefined) options = {};
        const transform = options.transform === undefined ? 'projective' : options.transform;
        if (transform !== 'projective' && transform !== 'affine') throw ("chainMatrices: options.transform must be 'projective' or 'affine'");
        const frames = options.frames;
        if (!Number.isInteger(frames) || frames < 0 || frames > 256) throw ("chainMatrices: options.frames must be an integer in 0..256");
        const anchor = options.anchor === undefined ? 0 : options.anchor;
        if (frames > 0 && (!Number.isInteger(anchor) || anchor < 0 || anchor >= frames)) throw ("chainMatrices: options.anchor must be a frame index");
        if (!(pairMatrices instanceof Float64Array) && !Array.isArray(pairMatrices)) throw ("chainMatrices: pairMatrices must be a Float64Array or an array of numbers");
        const pm = pairMatrices instanceof Float64Array ? pairMatrices : Float64Array.from(pairMatrices.flat());
        const P2 = this._bundlePairs('chainMatrices', pairs, frames);
        if (pm.length !== (P2.length / 2) * 8) throw ("chainMatrices: pairMatrices must hold 8 numbers per pair");
        if (frames === 0) return new Float64Array(0);
        return this._native.bundleChain(transform === 'projective' ? 1 : 0, frames, P2, pm, anchor);
    }

    /**
     * The inverse of a matrix in the layouts fitMatches() and bundleAdjust() use (hg_bundle_invert_matrix; host only): what turns a frame ->
     * canvas matrix into the canvas -> frame matrix the inverse warps take.  m: 8 numbers; options: { transform: 'projective' (default) |
     * 'affine' }.  Returns Float64Array(8); affine stays affine.
     */
    invertMatrix(m, options = {}) {
        if (options === null || options === undefined) options = {};
        const transform = options.transform === undefined ? 'projective' : options.transform;
        if (transform !== 'projective' && transform !== 'affine') throw ("invertMatrix: options.transform must be 'projective' or 'affine'");
        if ((!(m instanceof Float64Array) && !Array.isArray(m)) || m.length !== 8) throw ("invertMatrix: a matrix is 8 numbers");
        return this._native.bundleInvert(transform === 'projective' ? 1 : 0, m instanceof Float64Array ? m : Float64Array.from(m));
    }

    /**
     * The transforms fitMatches() returns, refined on the PIXELS of the two pictures (not part of the reference;
     * hg_align_refine_frames_device in include/hgwarp.h has the rules): Gauss-Newton on the intensity difference between every frame
     * (FROM) and the picture it was matched against (TO), started from `matrices`.  A local refinement: it needs a start within a few
     * pixels, or levels > 1, which walks both pictures' mip pyramids from the coarsest level down -- the planes and pyramids stay on the
     * device, only the matrices travel and are converted between levels (hg_align_scale_matrix).
     * fromImages: an array of F Uint8Arrays / Uint8ClampedArrays of width x height x channels bytes; toImages: an array of S of them
     * (toWidth x toHeight), 1 <= S <= F: frame f is aligned to picture f % S; matrices: Float64Array(8 F) or an array of 8 F numbers,
     * FROM -> TO, what fitMatches() returns.
     * options: { width, height, toWidth = width, toHeight = height, channels = 4 (or 1), transform: 'projective' (default) | 'affine',
     *            rect: [x, y, w, h] of the FROM picture (default: all of it), step = 2, iterations = 10, eps = 0.01 (pixels),
     *            photometric = true (fit a gain and a bias too), minValid (default: the number of parameters), levels = 1 }.
     * Returns { matrices: Float64Array(8 F) -- a frame that could not be refined keeps its input --, status: Int32Array(F) (0 converged,
     *           1 ran all iterations, 2 too few samples, 3 singular, 4 worse, 5 bad input; of level 0), updates: Int32Array(F),
     *           rms: Float64Array(F) (the final one), gains: Float64Array(2 F) (gain, bias per frame) }.
     * Needs no image and changes no state of the instance.  Throws a bare string for a bad option or a picture of the wrong size.
     */
    refineAlignment(fromImages, toImages, matrices, options = {}) {
        if (options === null || options === undefined) options = {};
        const isInt = (v, lo, hi) => Number.isInteger(v) && v >= lo && v <= hi;
        const transform = options.transform === undefined ? 'projective' : options.transform;
        if (transform !== 'projective' && transform !== 'affine') throw ("refineAlignment: options.transform must be 'projective' or 'affine'");
        const { width, height } = options;
        if (!isInt(width, 1, 32768) || !isInt(height, 1, 32768)) throw ("refineAlignment: options.width and options.height must be integers in 1..32768");
        const toWidth = options.toWidth === undefined ? width : options.toWidth, toHeight = options.toHeight === undefined ? height : options.toHeight;
        if (!isInt(toWidth, 1, 32768) || !isInt(toHeight, 1, 32768)) throw ("refineAlignment: options.toWidth and options.toHeight must be integers in 1..32768");
        const channels = options.channels === undefined ? 4 : options.channels;
        if (channels !== 1 && channels !== 4) throw ("refineAlignment: options.channels must be 1 or 4");
        const step = options.step === undefined ? 2 : options.step;
        if (!isInt(step, 1, 64)) throw ("refineAlignment: options.step must be an integer in 1..64");
        const iterations = options.iterations === undefined ? 10 : options.iterations;
        if (!isInt(iterations, 0, 64)) throw ("refineAlignment: options.iterations must be an integer in 0..64");
        const eps = options.eps === undefined ? 0.01 : options.eps;
        if (typeof eps !== 'number' || !Number.isFinite(eps) || eps < 0) throw ("refineAlignment: options.eps must be a finite number >= 0");
        const photometric = options.photometric === undefined ? true : !!options.photometric;
        const kind = transform === 'projective' ? 1 : 0;
        const P = (kind === 1 ? 8 : 6) + (photometric ? 2 : 0);
        const minValid = options.minValid === undefined ? P : options.minValid;
        if (!isInt(minValid, P, 0x7fffffff)) throw ("refineAlignment: options.minValid must be an integer >= " + P + " (the number of parameters)");
        const levels = options.levels === undefined ? 1 : options.levels;
        const sizes = [[width, height, toWidth, toHeight]];
        if (!isInt(levels, 1, 31)) throw ("refineAlignment: options.levels must be an integer >= 1");
        for (let k = 1; k < levels; k++) {
            const [w, h, tw, th] = sizes[k - 1];
            if (Math.max(w, h) === 1 || Math.max(tw, th) === 1) throw ("refineAlignment: options.levels must exist in both pictures' pyramids");
            sizes.push([(w + 1) >> 1, (h + 1) >> 1, (tw + 1) >> 1, (th + 1) >> 1]);
        }
        const rect = options.rect === undefined ? [0, 0, width, height] : Array.from(options.rect);
        if (rect.length !== 4 || !rect.every((v) => Number.isInteger(v)) || rect[0] < 0 || rect[1] < 0 || rect[2] < 1 || rect[3] < 1 || rect[0] + rect[2] > width || rect[1] + rect[3] > height)
            throw ("refineAlignment: options.rect must be [x, y, w, h], non-empty and inside the FROM picture");
        if (!Array.isArray(fromImages) || !Array.isArray(toImages)) throw ("refineAlignment: fromImages and toImages must be arrays of pictures");
        const F = fromImages.length, S = toImages.length;
        if (F > 4096) throw ("refineAlignment: at most 4096 frames");
        if (F > 0 && (S < 1 || S > F)) throw ("refineAlignment: toImages must hold 1..fromImages.length pictures");
        const pack = (imgs, w, h, name) => {
            const n = w * h * channels, out = new Uint8Array(imgs.length * n);
            imgs.forEach((im, f) => {
                if (!(im instanceof Uint8Array) && !(im instanceof Uint8ClampedArray)) throw ("refineAlignment: " + name + " " + f + " must be a Uint8Array or a Uint8ClampedArray");
                if (im.length !== n) throw ("refineAlignment: " + name + " " + f + " must hold width x height x channels bytes");
                out.set(im, f * n);
            });
            return out;
        };
        const from = pack(fromImages, width, height, 'fromImages'), to = pack(toImages, toWidth, toHeight, 'toImages');
        if (!(matrices instanceof Float64Array) && !Array.isArray(matrices)) throw ("refineAlignment: matrices must be a Float64Array or an array of 8 numbers per frame");
        let cur = Float64Array.from(matrices instanceof Float64Array ? matrices : matrices.flat(Infinity));
        if (cur.length !== 8 * F) throw ("refineAlignment: matrices must hold 8 numbers per frame");
        if (F === 0) return { matrices: new Float64Array(0), status: new Int32Array(0), updates: new Int32Array(0), rms: new Float64Array(0), gains: new Float64Array(0) };
        // the level-k pixels whose centres, x_0 = (x_k + 0.5) 2^k - 0.5, lie inside the rectangle
        const levelRect = (k, lw, lh) => {
            const lo = (a) => Math.ceil((2 * a + 1 - 2 ** k) / 2 ** (k + 1)), hi = (b) => Math.floor((2 * b - 1 - 2 ** k) / 2 ** (k + 1));
            const x0 = Math.max(lo(rect[0]), 0), y0 = Math.max(lo(rect[1]), 0);
            const x1 = Math.min(hi(rect[0] + rect[2]), lw - 1), y1 = Math.min(hi(rect[1] + rect[3]), lh - 1);
            return Int32Array.from([x0, y0, x1 - x0 + 1, y1 - y0 + 1]);
        };
        const job = this._native.alignBegin(this._ctx, from, width, height, F, to, toWidth, toHeight, S, channels, levels);
        try {
            let r = null;
            for (let k = levels - 1; k >= 0; k--) {
                const atK = k === 0 ? cur : this._native.alignScaleMatrix(kind, cur, 0, k);
                r = this._native.alignLevel(this._ctx, job, kind, k, levelRect(k, sizes[k][0], sizes[k][1]), step, photometric ? 1 : 0, iterations, eps, minValid, atK);
                cur = k === 0 ? r.matrices : this._native.alignScaleMatrix(kind, r.matrices, k, 0);
            }
            return { matrices: cur, status: r.status, updates: r.updates, rms: Float64Array.from({ length: F }, (_, f) => r.rms[2 * f + 1]), gains: r.gains };
        } finally {
            this._native.alignEnd(this._ctx, job);
        }
    }

    /**
     * The matches fitMatches() starts from: per frame the nearest train descriptor of every query descriptor, kept when it passes Lowe's
     * ratio test, the distance cap and, if asked for, the cross-check (not part of the reference; hg_match_descriptors_frames_device in
     * include/hgwarp.h has the rules, all of them exact).  querySets: an array of F Uint8Arrays of count_f x descBytes bytes; trainSets: an
     * array of S Uint8Arrays, 1 <= S <= max(F, 1): frame f is matched against train set f % S (one keyframe for all frames: S = 1).  The
     * counts may differ: the sets are padded to the longest (rows to a multiple of 16 bytes) and the device is told each set's count.
     * options: { kind: 'bits' (default; binary descriptors, Hamming distance) | 'u8' (byte vectors, squared L2), descBytes = 32 for 'bits',
     *            128 for 'u8', ratio = 0.8 (0: no ratio test), maxDistance = 0xffffffff (no cap), crossCheck = false,
     *            queryPoints / trainPoints: per set a Float32Array of x, y pairs or an array of [x, y], one per descriptor; both or none }.
     * Returns one record per frame: { count, pairs: Int32Array(2 count) of (query index, train index) in ascending query index,
     *                                 matches: Float32Array(4 count) of (x, y, u, v) = (query position, train position) -- with points only }.
     * The array of `matches` is what fitMatches() accepts as matchSets; its matrices map query -> train.
     * Needs no image and changes no state of the instance.  Throws a bare string for an unknown kind, a set whose length is not a multiple of
     * descBytes, a bad ratio, a bad maxDistance or points that do not fit their set.
     */
    matchDescriptors(querySets, trainSets, options = {}) {
        if (options === null || options === undefined) options = {};
        const kind = options.kind === undefined ? 'bits' : options.kind;
        if (kind !== 'bits' && kind !== 'u8') throw ("matchDescriptors: options.kind must be 'bits' or 'u8'");
        const descBytes = options.descBytes === undefined ? (kind === 'bits' ? 32 : 128) : options.descBytes;
        if (!Number.isInteger(descBytes) || descBytes < 1 || descBytes > 512) throw ("matchDescriptors: options.descBytes must be an integer in 1..512");
        const ratio = options.ratio === undefined ? 0.8 : options.ratio;
        if (typeof ratio !== 'number' || !(ratio >= 0 && ratio <= 1)) throw ("matchDescriptors: options.ratio must be a number in 0..1 (0: no ratio test)");
        const maxDistance = options.maxDistance === undefined ? 0xffffffff : options.maxDistance;
        if (!Number.isInteger(maxDistance) || maxDistance < 0 || maxDistance > 0xffffffff) throw ("matchDescriptors: options.maxDistance must be an integer in 0..2^32-1");
        const crossCheck = options.crossCheck === undefined ? false : !!options.crossCheck;
        if (!Array.isArray(querySets) || !Array.isArray(trainSets)) throw ("matchDescriptors: querySets and trainSets must be arrays of Uint8Arrays");
        if (querySets.length > 4096) throw ("matchDescriptors: at most 4096 frames");
        if (trainSets.length < 1 || trainSets.length > Math.max(querySets.length, 1)) throw ("matchDescriptors: trainSets must hold 1..max(frames, 1) sets");
        const stride = (descBytes + 15) & ~15;
        const pack = (sets, name) => {
            const counts = Int32Array.from(sets, (s, f) => {
                if (!(s instanceof Uint8Array)) throw ("matchDescriptors: " + name + " set " + f + " must be a Uint8Array");
                if (s.length % descBytes !== 0) throw ("matchDescriptors: " + name + " set " + f + " must hold rows of descBytes bytes");
                return s.length / descBytes;
            });
            const n = counts.reduce((m, c) => Math.max(m, c), 0);
            if (n > 65536) throw ("matchDescriptors: at most 65536 descriptors per set");
            const rows = new Uint8Array(sets.length * n * stride);
            sets.forEach((s, f) => { for (let i = 0; i < counts[f]; i++) rows.set(s.subarray(i * descBytes, (i + 1) * descBytes), (f * n + i) * stride); });
            return { counts, n, rows };
        };
        const q = pack(querySets, 'query'), t = pack(trainSets, 'train');
        const points = (lists, side, name) => {
            if (!Array.isArray(lists) || lists.length !== side.counts.length) throw ("matchDescriptors: options." + name + " must hold one list per set");
            const out = new Float32Array(side.counts.length * side.n * 2);
            lists.forEach((p, f) => {
                if (!(p instanceof Float32Array) && !Array.isArray(p)) throw ("matchDescriptors: options." + name + " list " + f + " must be a Float32Array or an array of [x, y]");
                const l = p instanceof Float32Array ? p : Float32Array.from(p.flat());
                if (l.length !== side.counts[f] * 2) throw ("matchDescriptors: options." + name + " list " + f + " must hold one x, y pair per descriptor");
                out.set(l, f * side.n * 2);
            });
            return out;
        };
        const hasQ = options.queryPoints !== undefined && options.queryPoints !== null, hasT = options.trainPoints !== undefined && options.trainPoints !== null;
        if (hasQ !== hasT) throw ("matchDescriptors: options.queryPoints and options.trainPoints come together");
        const qp = hasQ ? points(options.queryPoints, q, 'queryPoints') : null, tp = hasT ? points(options.trainPoints, t, 'trainPoints') : null;
        const r = this._native.matchDescriptors(this._ctx, kind === 'bits' ? 0 : 1, descBytes, stride, q.rows, q.n, q.counts, t.rows, t.n, t.counts, ratio, maxDistance,
                                                crossCheck ? 1 : 0, qp, tp);
        return querySets.map((s, f) => {
            const count = r.counts[f];
            const rec = { count, pairs: r.pairs.slice(f * q.n * 2, (f * q.n + count) * 2) };
            if (hasQ) rec.matches = r.matches.slice(f * q.n * 4, (f * q.n + count) * 4);
            return rec;
        });
    }

    /**
     * Thin-plate spline warps: the smooth interpolant through landmark pairs, where the piecewise affine transform kinks at every triangle
     * edge and ends at the hull of its mesh (not part of the reference; "thin-plate splines" in include/hgwarp.h has the rules).  One spline
     * per destiny point set, solved and evaluated on the device; only the results come down.
     * sourcePoints: the landmarks in the source picture, a Float32Array of x, y pairs or an array of [x, y] (3..1024 of them, in pixels);
     * destinyPointSets: an array of such lists, one per frame, where the landmarks go.
     * options: { smoothing = 0 (lambda >= 0 in the normalised frame; 0 interpolates), step = 1 (2, 4, 8, 16, 32: the spline is evaluated on
     *            a lattice and blended in between -- an approximation whose error sits around the landmarks),
     *            output = 'image' ('index' / 'coords': the source field itself, an Int32Array resp. a Float32Array of x, y pairs),
     *            sampling = 'nearest' ('bilinear'; pictures only),
     *            window: { x, y, width, height } for every frame, or an array of them (default: the integer bounding box of each destiny set),
     *            images: ImageData-shaped sources of one size, frame f reads images[f % images.length] (default: the instance's image) }.
     * Returns one record per frame: { data, width, height, x, y, status } -- status 0 ok, 1 singular (coincident or collinear landmarks),
     * 2 a coordinate that is not finite; a failed frame is empty (zero pixels, index -1, NaN coordinates).
     * Changes no state of the instance.  Throws a bare string for point lists that do not fit and options out of range.
     */
    warpThinPlate(sourcePoints, destinyPointSets, options = {}) {
        if (options === null || options === undefined) options = {};
        const list = (p, name) => {
            if (!(p instanceof Float32Array) && !Array.isArray(p)) throw ("warpThinPlate: " + name + " must be a Float32Array or an array of [x, y]");
            const l = p instanceof Float32Array ? p : Float32Array.from(p.flat());
            if (l.length % 2 !== 0) throw ("warpThinPlate: " + name + " must hold x, y pairs");
            return l;
        };
        const src = list(sourcePoints, 'sourcePoints'), N = src.length / 2;
        if (N < 3 || N > 1024) throw ("warpThinPlate: 3 to 1024 landmarks are needed, but " + N + " were given");
        if (!Array.isArray(destinyPointSets)) throw ("warpThinPlate: destinyPointSets must be an array of point lists");
        const F = destinyPointSets.length;
        if (F > 4096) throw ("warpThinPlate: at most 4096 frames");
        const dst = new Float32Array(F * N * 2);
        destinyPointSets.forEach((p, f) => {
            const l = list(p, 'destiny point set ' + f);
            if (l.length !== 2 * N) throw (`It must be the same amount of destiny points (${l.length / 2}) than source points (${N})`);
            dst.set(l, f * N * 2);
        });
        const smoothing = options.smoothing === undefined ? 0 : options.smoothing;
        if (typeof smoothing !== 'number' || !Number.isFinite(smoothing) || smoothing < 0) throw ("warpThinPlate: options.smoothing must be a finite number >= 0");
        const step = options.step === undefined ? 1 : options.step;
        if (![1, 2, 4, 8, 16, 32].includes(step)) throw ("warpThinPlate: options.step must be 1, 2, 4, 8, 16 or 32");
        const output = options.output === undefined ? 'image' : options.output;
        if (output !== 'image' && output !== 'index' && output !== 'coords') throw ("warpThinPlate: options.output must be 'image', 'index' or 'coords'");
        const sampling = options.sampling === undefined ? 'nearest' : options.sampling;
        if (sampling !== 'nearest' && sampling !== 'bilinear') throw ("warpThinPlate: options.sampling must be 'nearest' or 'bilinear'");
        const isInt = (v) => Number.isInteger(v) && Math.abs(v) <= 0x7fffffff;
        const windows = new Int32Array(4 * F);
        for (let f = 0; f < F; f++) {
            let w = Array.isArray(options.window) ? options.window[f] : options.window;
            if (Array.isArray(options.window) && options.window.length !== F) throw ("warpThinPlate: options.window must hold one window per frame");
            if (w === undefined || w === null) {
                let x0 = Infinity, y0 = Infinity, x1 = -Infinity, y1 = -Infinity, finite = true;
                for (let i = 0; i < N; i++) {
                    const x = dst[(f * N + i) * 2], y = dst[(f * N + i) * 2 + 1];
                    finite = finite && Number.isFinite(x) && Number.isFinite(y);
                    if (x < x0) x0 = x; if (x > x1) x1 = x; if (y < y0) y0 = y; if (y > y1) y1 = y;
                }
                w = finite ? { x: Math.floor(x0), y: Math.floor(y0), width: Math.ceil(x1) - Math.floor(x0) + 1, height: Math.ceil(y1) - Math.floor(y0) + 1 }
                                                       : { x: 0, y: 0, width: 0, height: 0 };      // (a coordinate that is not finite: the frame fails, its window is empty)
            }
            if (!w || !isInt(w.x) || !isInt(w.y) || !isInt(w.width) || !isInt(w.height)) throw ("warpThinPlate: options.window must be { x, y, width, height }, four integers");
            windows.set([w.x, w.y, Math.max(w.width, 0), Math.max(w.height, 0)], 4 * f);
        }
        let W = this._width, H = this._height, planes = null, nImages = 0;
        if (options.images !== undefined && options.images !== null) {
            const images = options.images;
            if (!Array.isArray(images) || images.length === 0) throw ("warpThinPlate: options.images needs a non-empty array of ImageData-shaped sources");
            W = images[0] ? images[0].width : 0; H = images[0] ? images[0].height : 0;
            for (const im of images)
                if (!im || !ArrayBuffer.isView(im.data) || im.width !== W || im.height !== H || im.data.length !== W * H * 4)
                    throw ("warpThinPlate: every image must be ImageData-shaped RGBA and of one size");
            if (output === 'image') {
                planes = new Uint8Array(images.length * W * H * 4);
                images.forEach((im, k) => planes.set(im.data, k * W * H * 4));
                nImages = images.length;
            }
        } else if (output === 'image') {
            if (this._image === null) throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");
            planes = new Uint8Array(this._image.buffer, this._image.byteOffset, this._image.length);
            nImages = 1;
        }
        if (!Number.isInteger(W) || !Number.isInteger(H) || W < 1 || H < 1) throw ("warpThinPlate: the source size is not known: give options.images or set an image first");
        const code = output === 'image' ? (sampling === 'bilinear' ? 1 : 0) : (output === 'index' ? 2 : 3);
        const r = this._native.warpThinPlate(this._ctx, dst, F, src, 1, N, windows, smoothing, step, code, planes, W, H, nImages);
        const px = code === 3 ? 8 : 4;
        let off = 0;
        return destinyPointSets.map((p, f) => {
            const width = windows[4 * f + 2], height = windows[4 * f + 3], bytes = width * height * px;
            const b = r.data.buffer.slice(r.data.byteOffset + off, r.data.byteOffset + off + bytes);
            off += (bytes + 255) & ~255;
            const data = code === 2 ? new Int32Array(b) : code === 3 ? new Float32Array(b) : new Uint8ClampedArray(b);
            return { data, width, height, x: windows[4 * f], y: windows[4 * f + 1], status: r.status[f] };
        });
    }

    /**
     * Frames projected onto a plane, a cylinder or a sphere from a camera per frame: what a panorama wider than about 100 degrees needs,
     * and the only way to say "this picture was taken with k1 = -0.2" (not part of the reference; "camera models" in include/hgwarp.h has
     * the rules).  The fields are written and the pictures gathered on the device; only the results come down.
     * cameras: one per frame, { rotation: 9 numbers (row-major, camera <- world) or three rows of three, focal: f or [fx, fy],
     *          principal: [cx, cy] (default: the centre of the source), distortion: [k1, k2, p1, p2, k3] (default: none) }.
     * options: { surface = 'sphere' ('plane' / 'cylinder'), scale (required: pixels per radian; for the plane the canvas focal length),
     *            center = [0, 0] (the canvas position of azimuth 0, elevation 0),
     *            window: { x, y, width, height } for every frame, or an array of them (default: hg_camera_limits of each camera),
     *            sampling = 'nearest' ('bilinear'; pictures only), output = 'image' ('index' / 'coords': the source field itself),
     *            images: ImageData-shaped sources of one size, frame f reads images[f % images.length] (default: the instance's image) }.
     * Returns one record per frame: { data, width, height, x, y }; pixels no camera ray reaches are empty (zero pixels, index -1, NaN
     * coordinates).  Changes no state of the instance.  Throws a bare string for cameras that do not fit and options out of range.
     */
    warpCamera(cameras, options = {}) {
        if (options === null || options === undefined) options = {};
        if (!Array.isArray(cameras)) throw ("warpCamera: cameras must be an array of { rotation, focal, principal, distortion }");
        const F = cameras.length;
        if (F > 4096) throw ("warpCamera: at most 4096 frames");
        const surface = options.surface === undefined ? 'sphere' : options.surface;
        const surfaceCode = ['plane', 'cylinder', 'sphere'].indexOf(surface);
        if (surfaceCode < 0) throw ("warpCamera: options.surface must be 'plane', 'cylinder' or 'sphere'");
        const scale = options.scale;
        if (typeof scale !== 'number' || !Number.isFinite(scale) || scale <= 0) throw ("warpCamera: options.scale must be a finite number > 0 (pixels per radian)");
        const center = options.center === undefined ? [0, 0] : options.center;
        if (!Array.isArray(center) || center.length !== 2 || !center.every((v) => typeof v === 'number' && Number.isFinite(v))) throw ("warpCamera: options.center must be [u0, v0], two finite numbers");
        const output = options.output === undefined ? 'image' : options.output;
        if (output !== 'image' && output !== 'index' && output !== 'coords') throw ("warpCamera: options.output must be 'image', 'index' or 'coords'");
        const sampling = options.sampling === undefined ? 'nearest' : options.sampling;
        if (sampling !== 'nearest' && sampling !== 'bilinear') throw ("warpCamera: options.sampling must be 'nearest' or 'bilinear'");
        let W = this._width, H = this._height, planes = null, nImages = 0;
        if (options.images !== undefined && options.images !== null) {
            const images = options.images;
            if (!Array.isArray(images) || images.length === 0) throw ("warpCamera: options.images needs a non-empty array of ImageData-shaped sources");
            W = images[0] ? images[0].width : 0; H = images[0] ? images[0].height : 0;
            for (const im of images)
                if (!im || !ArrayBuffer.isView(im.data) || im.width !== W || im.height !== H || im.data.length !== W * H * 4)
                    throw ("warpCamera: every image must be ImageData-shaped RGBA and of one size");
            if (output === 'image') {
                planes = new Uint8Array(images.length * W * H * 4);
                images.forEach((im, k) => planes.set(im.data, k * W * H * 4));
                nImages = images.length;
            }
        } else if (output === 'image') {
            if (this._image === null) throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");
            planes = new Uint8Array(this._image.buffer, this._image.byteOffset, this._image.length);
            nImages = 1;
        }
        if (!Number.isInteger(W) || !Number.isInteger(H) || W < 1 || H < 1) throw ("warpCamera: the source size is not known: give options.images or set an image first");
        const records = new Float64Array(F * 32);
        cameras.forEach((c, f) => records.set(this._cameraRecord('warpCamera', c, f, W, H), f * 32));
        const isInt = (v) => Number.isInteger(v) && Math.abs(v) <= 0x7fffffff;
        if (Array.isArray(options.window) && options.window.length !== F) throw ("warpCamera: options.window must hold one window per frame");
        const windows = new Int32Array(4 * F);
        for (let f = 0; f < F; f++) {
            let w = Array.isArray(options.window) ? options.window[f] : options.window;
            if (w === undefined || w === null) {
                const l = this._native.cameraLimits(records.subarray(f * 32, f * 32 + 32), W, H, surfaceCode, scale, center[0], center[1]);
                w = { x: l[0], y: l[1], width: l[2], height: l[3] };
            }
            if (!w || !isInt(w.x) || !isInt(w.y) || !isInt(w.width) || !isInt(w.height)) throw ("warpCamera: options.window must be { x, y, width, height }, four integers");
            windows.set([w.x, w.y, Math.max(w.width, 0), Math.max(w.height, 0)], 4 * f);
        }
        const code = output === 'image' ? (sampling === 'bilinear' ? 1 : 0) : (output === 'index' ? 2 : 3);
        const r = this._native.warpCamera(this._ctx, records, windows, surfaceCode, scale, center[0], center[1], code, planes, W, H, nImages);
        const px = code === 3 ? 8 : 4;
        let off = 0;
        return cameras.map((c, f) => {
            const width = windows[4 * f + 2], height = windows[4 * f + 3], bytes = width * height * px;
            const b = r.data.buffer.slice(r.data.byteOffset + off, r.data.byteOffset + off + bytes);
            off += (bytes + 255) & ~255;
            const data = code === 2 ? new Int32Array(b) : code === 3 ? new Float32Array(b) : new Uint8ClampedArray(b);
            return { data, width, height, x: windows[4 * f], y: windows[4 * f + 1] };
        });
    }

    /** The 32-double record of one camera of warpCamera (hg_camera_pack_record), after the class's own checks of its shape. */
    _cameraRecord(who, c, f, W, H) {
        if (c === null || typeof c !== 'object') throw (who + ": camera " + f + " must be { rotation, focal, principal, distortion }");
        const rot = Array.isArray(c.rotation) ? c.rotation.flat() : c.rotation;
        if ((!Array.isArray(rot) && !(rot instanceof Float64Array)) || rot.length !== 9 || !Array.from(rot).every((v) => typeof v === 'number'))
            throw (who + ": camera " + f + ": rotation must be 9 numbers, row-major, or three rows of three");
        const fo = typeof c.focal === 'number' ? [c.focal, c.focal] : c.focal;
        if (!Array.isArray(fo) || fo.length !== 2 || !fo.every((v) => typeof v === 'number' && Number.isFinite(v) && v > 0))
            throw (who + ": camera " + f + ": focal must be a finite number > 0 or [fx, fy]");
        const pp = c.principal === undefined ? [W / 2, H / 2] : c.principal;
        if (!Array.isArray(pp) || pp.length !== 2 || !pp.every((v) => typeof v === 'number' && Number.isFinite(v)))
            throw (who + ": camera " + f + ": principal must be [cx, cy], two finite numbers");
        let dist = null;
        if (c.distortion !== undefined && c.distortion !== null) {
            if (!Array.isArray(c.distortion) || c.distortion.length !== 5 || !c.distortion.every((v) => typeof v === 'number' && Number.isFinite(v)))
                throw (who + ": camera " + f + ": distortion must be [k1, k2, p1, p2, k3], five finite numbers");
            dist = Float64Array.from(c.distortion);
        }
        return this._native.cameraPackRecord(Float64Array.from(rot), fo[0], fo[1], pp[0], pp[1], dist, W, H);
    }

    /**
     * From homographies to cameras: the focal lengths and the rotation a homography between two pictures of one rotating camera implies
     * (hg_camera_focals_from_matrix, hg_camera_rotation_from_matrix).  matrix: 9 numbers, row-major, or the 8 of this library's projective
     * matrices (h8 = 1), x_to ~ H x_from in PIXEL coordinates.
     * options: { principalFrom = [0, 0], principalTo = [0, 0] (the principal points; the focal lengths are estimated in coordinates relative
     *            to them), focalFrom, focalTo (numbers or [fx, fy]: skip the estimate of that side) }.
     * Returns { focalFrom, focalTo, okFrom, okTo, rotation } -- rotation: Float64Array(9), TO camera <- FROM camera, or null when a focal
     * length is neither given nor estimable (a rotation about the optical axis says nothing about it).
     */
    cameraFromMatrices(matrix, options = {}) {
        if (options === null || options === undefined) options = {};
        if ((!Array.isArray(matrix) && !(matrix instanceof Float64Array)) || (matrix.length !== 9 && matrix.length !== 8) || !Array.from(matrix).every((v) => typeof v === 'number' && Number.isFinite(v)))
            throw ("cameraFromMatrices: a matrix is 9 (or 8) finite numbers");
        const m = Float64Array.from(matrix.length === 9 ? matrix : [...matrix, 1]);
        const point = (p, name) => {
            const v = p === undefined ? [0, 0] : p;
            if (!Array.isArray(v) || v.length !== 2 || !v.every((t) => typeof t === 'number' && Number.isFinite(t))) throw ("cameraFromMatrices: options." + name + " must be [cx, cy], two finite numbers");
            return v;
        };
        const focal = (v, name) => {
            if (v === undefined || v === null) return null;
            const fo = typeof v === 'number' ? [v, v] : v;
            if (!Array.isArray(fo) || fo.length !== 2 || !fo.every((t) => typeof t === 'number' && Number.isFinite(t) && t > 0)) throw ("cameraFromMatrices: options." + name + " must be a finite number > 0 or [fx, fy]");
            return fo;
        };
        const pf = point(options.principalFrom, 'principalFrom'), pt = point(options.principalTo, 'principalTo');
        let ff = focal(options.focalFrom, 'focalFrom'), ft = focal(options.focalTo, 'focalTo');
        // the matrix between coordinates relative to the principal points: T_to^-1 H T_from, T = the shift by the principal point
        const c = new Float64Array(9);
        for (let r = 0; r < 3; r++) { c[3 * r] = m[3 * r]; c[3 * r + 1] = m[3 * r + 1]; c[3 * r + 2] = m[3 * r] * pf[0] + m[3 * r + 1] * pf[1] + m[3 * r + 2]; }
        for (let k = 0; k < 3; k++) { c[k] -= pt[0] * c[6 + k]; c[3 + k] -= pt[1] * c[6 + k]; }
        const e = this._native.cameraFocals(c);
        const okFrom = ff !== null || e[2] === 1, okTo = ft !== null || e[3] === 1;
        if (ff === null && e[2] === 1) ff = [e[0], e[0]];
        if (ft === null && e[3] === 1) ft = [e[1], e[1]];
        let rotation = null;
        if (okFrom && okTo) rotation = this._native.cameraRotation(m, Float64Array.from([ff[0], ff[1], pf[0], pf[1]]), Float64Array.from([ft[0], ft[1], pt[0], pt[1]]));
        return { focalFrom: ff === null ? null : (ff[0] === ff[1] ? ff[0] : ff), focalTo: ft === null ? null : (ft[0] === ft[1] ? ft[0] : ft), okFrom, okTo, rotation };
    }

    /**
     * Dense optical flow between pairs of pictures: a per-pixel, non-parametric registration for what a homography cannot follow --
     * parallax, a rolling shutter, things that move (not part of the reference; hg_flow_dense_frames_device in include/hgwarp.h has the
     * rule, pyramidal Lucas-Kanade with integer window sums, exact to the bit).
     * fromImages / toImages: arrays of Uint8Arrays of equal size, width x height x channels bytes each; picture f of fromImages is
     * registered onto picture f % toImages.length of toImages.
     * options: { width, height (required), channels = 4 (RGBA; 1: grey), levels (default: as many as leave the coarsest level at least 16
     *            pixels on its shorter side), iterations = 4 (1..32 per level), radius = 3 (1..7: the window is 2 radius + 1 pixels a side),
     *            minEig = 1 (>= 0: the smallest per-pixel gradient eigenvalue a window may have and still be solved), maxUpdate = 1 ((0, 4]:
     *            the cap on the change of one iteration, pixels), residual = false, good = false, warp = false,
     *            field (default: true without warp, false with it) }.
     * Returns { field, width, height, frames, residual?, good?, images? }: field is a Float32Array of frames x width x height x, y pairs
     * over toImages' pixel grid whose values are positions in the FROM picture (NaN where they leave it) -- what the remaps and the
     * mosaics read --, or null when it was not asked for; residual and good one byte per pixel; images (warp: true) the FROM pictures sent
     * through the field by the bilinear remap on the device, one Uint8Array per frame.
     * Needs no image and changes no state of the instance.  Throws a bare string for pictures of the wrong size and options out of range.
     */
    denseFlow(fromImages, toImages, options = {}) {
        if (options === null || options === undefined) options = {};
        const isInt = (v) => Number.isInteger(v);
        const W = options.width, H = options.height;
        if (!isInt(W) || !isInt(H) || W < 1 || H < 1 || W > 32768 || H > 32768 || W * H > 2 ** 30) throw ("denseFlow: options.width and options.height must be integers in 1..32768");
        const channels = options.channels === undefined ? 4 : options.channels;
        if (channels !== 1 && channels !== 4) throw ("denseFlow: options.channels must be 1 or 4");
        let top = 1;
        for (let w = W, h = H; w > 1 || h > 1; top++) { w = (w + 1) >> 1; h = (h + 1) >> 1; }
        let levels = options.levels;
        if (levels === undefined) {
            levels = 1;
            for (let s = Math.min(W, H); levels < 12 && ((s + 1) >> 1) >= 16; levels++) s = (s + 1) >> 1;
        }
        if (!isInt(levels) || levels < 1 || levels > Math.min(top, 12)) throw ("denseFlow: options.levels must be an integer in 1.." + Math.min(top, 12));
        const iterations = options.iterations === undefined ? 4 : options.iterations;
        if (!isInt(iterations) || iterations < 1 || iterations > 32) throw ("denseFlow: options.iterations must be an integer in 1..32");
        const radius = options.radius === undefined ? 3 : options.radius;
        if (!isInt(radius) || radius < 1 || radius > 7) throw ("denseFlow: options.radius must be an integer in 1..7");
        const minEig = options.minEig === undefined ? 1 : options.minEig;
        if (typeof minEig !== 'number' || !Number.isFinite(minEig) || minEig < 0) throw ("denseFlow: options.minEig must be a finite number >= 0");
        const maxUpdate = options.maxUpdate === undefined ? 1 : options.maxUpdate;
        if (typeof maxUpdate !== 'number' || !(maxUpdate > 0) || !(maxUpdate <= 4)) throw ("denseFlow: options.maxUpdate must lie in (0, 4]");
        const plane = W * H * channels;
        const pack = (images, name) => {
            if (!Array.isArray(images)) throw ("denseFlow: " + name + " must be an array of Uint8Arrays");
            const all = new Uint8Array(images.length * plane);
            images.forEach((im, k) => {
                if (!(im instanceof Uint8Array) && !(im instanceof Uint8ClampedArray)) throw ("denseFlow: " + name + "[" + k + "] must be a Uint8Array");
                if (im.length !== plane) throw ("denseFlow: " + name + "[" + k + "] must hold width x height x channels = " + plane + " bytes, but holds " + im.length);
                all.set(im, k * plane);
            });
            return all;
        };
        const from = pack(fromImages, 'fromImages'), to = pack(toImages, 'toImages');
        const F = fromImages.length, S = toImages.length;
        if (F > 4096) throw ("denseFlow: at most 4096 frames");
        if (S < 1 || S > Math.max(F, 1)) throw ("denseFlow: toImages must hold between 1 and fromImages.length pictures");
        const warp = options.warp === true;
        const wantField = options.field === undefined ? !warp : options.field === true;
        const flags = (wantField ? 1 : 0) | (options.residual === true ? 2 : 0) | (options.good === true ? 4 : 0) | (warp ? 8 : 0);
        const r = this._native.denseFlow(this._ctx, from, to, W, H, channels, F, S, levels, iterations, radius, minEig, maxUpdate, flags);
        const out = { field: r.field, width: W, height: H, frames: F };
        if (options.residual === true) out.residual = r.residual;
        if (options.good === true) out.good = r.good;
        if (warp) out.images = Array.from({ length: F }, (_, f) => r.images.slice(f * plane, (f + 1) * plane));
        return out;
    }

    /**
     * The descriptors matchDescriptors() starts from: the keypoints of a set of pictures -- Harris corners in integer arithmetic, the best
     * perCell of every cell x cell cell of the picture, an orientation and a 256-bit binary descriptor each (not part of the reference;
     * hg_detect_describe_frames_device in include/hgwarp.h has the rules, all of them exact).  It is not ORB: both sides of a match have to
     * come from this call.  It is single-scale.  images: an array of Uint8Arrays of equal size, width x height x channels bytes each.
     * options: { width, height (required), channels = 4 (RGBA; 1: grey), cell = 32 (8..256), perCell = 2 (1..16), minResponse = 1e10 (an
     *            integer in 1..2^53: the smallest corner response kept.  The default is a guess: on the numpy model thresholds from 1 to 1e13
     *            changed the keypoint count of a textured 192 x 160 scene by under 20 %; nobody has measured it on photographs) }.
     * Returns one record per picture: { count, points: Float32Array(2 count) of x, y, descriptors: Uint8Array(32 count) } -- what
     * matchDescriptors() takes as a query or train set (kind 'bits', descBytes 32) and as queryPoints / trainPoints.
     * Needs no image and changes no state of the instance.  Throws a bare string for pictures of the wrong size and options out of range.
     */
    detectAndDescribe(images, options = {}) {
        if (options === null || options === undefined) options = {};
        const { width, height } = options;
        if (!Number.isInteger(width) || !Number.isInteger(height) || width < 1 || height < 1 || width > 32768 || height > 32768) throw ("detectAndDescribe: options.width and options.height must be integers in 1..32768");
        const channels = options.channels === undefined ? 4 : options.channels;
        if (channels !== 1 && channels !== 4) throw ("detectAndDescribe: options.channels must be 1 or 4");
        const cell = options.cell === undefined ? 32 : options.cell;
        if (!Number.isInteger(cell) || cell < 8 || cell > 256) throw ("detectAndDescribe: options.cell must be an integer in 8..256");
        const perCell = options.perCell === undefined ? 2 : options.perCell;
        if (!Number.isInteger(perCell) || perCell < 1 || perCell > 16) throw ("detectAndDescribe: options.perCell must be an integer in 1..16");
        const minResponse = options.minResponse === undefined ? 1e10 : options.minResponse;
        if (!Number.isInteger(minResponse) || minResponse < 1 || minResponse > 2 ** 53) throw ("detectAndDescribe: options.minResponse must be an integer in 1..2^53");
        if (Math.ceil(width / cell) * Math.ceil(height / cell) * perCell > 65536) throw ("detectAndDescribe: at most 65536 keypoint slots per picture (cells x perCell)");
        if (!Array.isArray(images)) throw ("detectAndDescribe: images must be an array of Uint8Arrays");
        if (images.length > 4096) throw ("detectAndDescribe: at most 4096 pictures");
        const plane = width * height * channels;
        const planes = new Uint8Array(images.length * plane);
        images.forEach((im, f) => {
            if (!(im instanceof Uint8Array) && !(im instanceof Uint8ClampedArray)) throw ("detectAndDescribe: picture " + f + " must be a Uint8Array");
            if (im.length !== plane) throw ("detectAndDescribe: picture " + f + " must hold width x height x channels bytes");
            planes.set(im, f * plane);
        });
        const r = this._native.detectAndDescribe(this._ctx, planes, images.length, width, height, channels, cell, perCell, minResponse);
        return images.map((im, f) => {
            const count = r.counts[f];
            return { count, points: r.points.slice(f * r.nSlots * 2, (f * r.nSlots + count) * 2),
                     descriptors: r.descriptors.slice(f * r.nSlots * 32, (f * r.nSlots + count) * 32) };
        });
    }

    /**
     * What sourceField() and remap() share: which field entry point of the addon the current state and options.loop lead to, with its
     * arguments after the context -- { entry, args, width, height }; the addon's functions are 'field' + entry and 'remap' + entry -- after
     * the refusals, the solves and the uploads that field needs.  null: the window is empty.  fmt: 0 = index, 1 = coords.
     */
    _fieldCall(who, fmt, options) {
        const loop = options === null || options === undefined || options.loop === undefined ? 'inverse' : options.loop;
        if (loop !== 'inverse' && loop !== 'warp' && loop !== 'forward') throw (who + ": options.loop must be 'inverse', 'warp' or 'forward'");
        if (this._image === null) throw (who + "() needs an image: call `setImage(img)` or `setSourcePoints(points, img)` first");
        const [xo, yo, ow, oh] = this._window();
        let entry, args;
        if (loop === 'forward' || (loop === 'warp' && this._dispatchesForward())) {
            if (fmt !== 0) throw (who === 'remap' ? "remap: a forward loop remaps 'nearest' only (it copies whole pixels from integer positions)"
                                                  : "sourceField: a forward loop has an 'index' field only (it copies whole pixels from integer positions)");
            if (this.transform === 'piecewiseaffine') {
                if (!(this.repairStaleMap || (this._mapIsCurrentForward() && this._matricesAreCurrent())))
                    throw (who + ": the forward loop would read a stale map or matrices of an older point set (call setSourcePoints / setDestinyPoints first)");
                if (!(ow * oh >= 1)) return null;
                checkedMapLength(ow * oh);
                this._uploadImage();
                this._uploadMesh();
                entry = 'ForwardPiecewise'; args = [asF32(this._dstPoints), this._maxSrcX, this._maxSrcY, xo, yo, ow, oh];
            } else {
                if (!(ow * oh >= 1)) return null;
                checkedMapLength(ow * oh);
                this._uploadImage();
                entry = 'ForwardGeometric'; args = [this.transform === 'affine' ? AFFINE : PROJECTIVE, Float64Array.from(this._transformMatrix), xo, yo, ow, oh];
            }
        } else if (this.transform === 'piecewiseaffine') {
            if (!(this.repairStaleMap || this._matricesAreCurrent()))
                throw (who + ": the piecewise matrices belong to an older point set (call setDestinyPoints first)");
            if (!(ow * oh >= 1)) return null;
            checkedMapLength(ow * oh);
            this._uploadImage();
            this._uploadMesh();
            this._native.piecewisePrepare(this._ctx, asF32(this._dstPoints), xo, yo, ow, oh);
            entry = 'InversePiecewise'; args = [fmt];
        } else {
            this._alignRanges();
            const inv = this._solve(this._dstPoints, this._srcPoints);
            if (!(ow * oh >= 1)) return null;
            checkedMapLength(ow * oh);
            this._uploadImage();
            entry = 'InverseGeometric'; args = [this.transform === 'affine' ? AFFINE : PROJECTIVE, Float64Array.from(inv), xo, yo, ow, oh, fmt];
        }
        return { entry, args, width: ow, height: oh };
    }

    /**
     * The benchmarked caller loop `for (f) { setDestinyPoints(dst[f]); warp(); }` (test/benchmark.js:107-110) as GPU batches.
     * dstPointSets: array of point sets.  Returns an array of ImageData-shaped frames, frame f identical to what the loop returns
     * for it -- INCLUDING warp()'s choice between the inverse and the forward (scatter-semantics) loop, made per frame on that
     * frame's output window exactly as warp() makes it (:421-422 piecewise, :426-427 affine, :431 projective): the frames that
     * dispatch inverse go through one inverse batch, the ones that dispatch forward through one forward batch.
     * options: {inverse: true} = the loop with warp(null, false, true) (applyAlwaysInverse: every frame through the inverse loop);
     *          {images: [...]} = the loop warp(image_f) (frame f reads images[f % images.length]); {devices: [...]} = the inverse
     *          frames spread over several GPUs of this node (forward frames run on this instance's own device);
     *          {pointsAreNormalized: bool} = the second argument of every setDestinyPoints (default: the reference's auto-detect).
     *          {reuseBatchOutput: true} (or the constructor option of that name) = the frames are views of one buffer of this instance that
     *          the next warpBatch() overwrites (see below); {ownFrames: true} overrides it for one call.
     * Every setDestinyPoints(dst[f]) runs on the host exactly as in the loop (normalisation auto-detect, in-place scaling of typed
     * arrays, window derivation), so the instance ends in the state the loop would leave it in.
     * LIFE TIME OF THE FRAMES: by default every frame owns its buffer (a pooled page-locked one while the pool has room, else a V8 array),
     * exactly like the frames the reference's loop returns -- a caller may accumulate them across calls.  With `reuseBatchOutput` (opt-in,
     * like `reuseOutput` for warp()) the frames of a batch are views of ONE page-locked buffer owned by this instance, reused by the next
     * warpBatch() on it: consume (or copy) a batch before asking for the next one.  The returned array then has a `release()` method that
     * gives the buffer back at once (the frames become empty), and nothing depends on when V8 collects garbage: no 34-MB allocation per 4K
     * frame, no fall-back to plain arrays in a loop that never yields (plain `node`, 4K, batches of 8: 0.73 instead of 2.05 ms per frame).
     * The slab counts against Homography.setPinnedLimit(); when it does not fit (or the limit is 0) the batch silently gets own frames.
     * With {images} the pass is pipelined: the upload of source f + 1 overlaps the download of frame f.
     * {sourcePoints: [...]} (piecewise only; one source point set per destiny point set) = the loop
     *     for (f) { setSourcePoints(src[f]); setDestinyPoints(dst[f]); warp(image_f); }
     * -- every frame's landmarks live in its own image -- see _warpBatchMoving.
     */
    warpBatch(dstPointSets, options = {}) {
        if (options.sourcePoints !== undefined && options.sourcePoints !== null) return this._warpBatchMoving(dstPointSets, options);
        if (this.transform === 'affine' || this.transform === 'projective') return this._warpBatchGeometric(dstPointSets, options);
        if (this.transform !== 'piecewiseaffine') throw ("hgwarp: warpBatch() needs a transform (set the source points first)");
        const F = dstPointSets.length, n = this._srcPoints.length;
        const all = new Float32Array(F * n), geoms = new Int32Array(F * 4), forward = new Array(F).fill(false), blank = new Array(F).fill(false);
        const stale = [];                                       // forward frames that read something else than the forward map of the current mesh (:957)
        for (let f = 0; f < F; f++) {
            this.setDestinyPoints(dstPointSets[f], options.pointsAreNormalized === undefined ? null : options.pointsAreNormalized);   // :337-380, as the loop does
            if (this._image === null && !options.images) throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");   // the loop's first warp() (:411-413)
            all.set(asF32(this._dstPoints), f * n);
            const [xo, yo, ow, oh] = this._window();
            forward[f] = !(options.inverse === true || this._sampling === 'bilinear' || ow > this._width || oh > this._height || ow * 1.2 < this._width || oh * 1.2 < this._height);   // :421-422
            blank[f] = !(ow * oh >= 1);                                                                 // :440: a 1 x 1 blank frame
            // the shared map field, carried from frame to frame as the loop would: an inverse frame leaves its own map there (:847-857),
            // a forward frame reads what it finds
            if (!forward[f]) {
                checkedMapLength(ow * oh);
                this._map = { kind: 'inverse', pts: all.subarray(f * n, (f + 1) * n), tris: this._triangles, width: ow, height: oh, yOff: yo };
            } else if (this.repairStaleMap) {
                if (!this._mapIsCurrentForward()) this._snapshotForwardMap();
            } else if (!(this._mapIsCurrentForward() && this._matricesAreCurrent())) {
                if (this._map === null) throw new TypeError("Cannot read property '0' of null");
                stale.push({ f, map: this._map, mats: this._snapshotMatrices(), blank: blank[f] });     // (a blank one too: its loop still reads the held map, :957-961)
                blank[f] = blank[f] || null;                                                            // (null: neither blank nor batched)
            }
            if (blank[f] === true) continue;
            checkedLength(ow * oh * 4);
            geoms.set([xo, yo, ow, oh], f * 4);
        }
        const frames = new Array(F).fill(null);
        const pick = (want) => { const ids = []; for (let f = 0; f < F; f++) if (blank[f] === false && forward[f] === want) ids.push(f); return ids; };
        const subset = (ids) => {                                                                       // points / windows / sources of a subset of the frames
            if (ids.length === F) return { pts: all, g: geoms, images: options.images };
            const pts = new Float32Array(ids.length * n), g = new Int32Array(ids.length * 4);
            ids.forEach((f, k) => { pts.set(all.subarray(f * n, (f + 1) * n), k * n); g.set(geoms.subarray(4 * f, 4 * f + 4), 4 * k); });
            const images = options.images ? ids.map((f) => options.images[f % options.images.length]) : options.images;
            return { pts, g, images };
        };
        const own = options.ownFrames === true || !(options.reuseBatchOutput === undefined ? this.reuseBatchOutput : options.reuseBatchOutput === true);
        const room = (g) => { if (!own) return; let largest = 0; for (let k = 0; k < g.length / 4; k++) largest = Math.max(largest, g[4 * k + 2] * g[4 * k + 3] * 4); makeRoomFor(this._native, largest, g.length / 4); };
        const inv = pick(false), fwd = pick(true);
        if (inv.length) {
            const { pts, g, images } = subset(inv);
            room(g);
            let datas;
            if (options.devices !== undefined && options.devices !== null) {
                // several GPUs of this node: device i of G warps a contiguous block of the frames (hg_multi_*: no collective on the
                // data path; the shared source is fanned out once over xGMI peer copies -- or, with {images}, every device uploads the
                // sources of its own block and nothing is exchanged at all)
                const multi = this._multiFor(options.devices);
                const tris = this._triangles instanceof Uint32Array ? this._triangles : Uint32Array.from(this._triangles);
                this._native.multiSetMesh(multi, asF32(this._srcPoints), tris, this._minSrcX, this._minSrcY);
                if (images) {
                    datas = this._native.multiWarpBatch(multi, pts, g, this._checkedSources(images), this._width, this._height);
                    this._multiImage = null;                                                             // (the devices now hold the per-frame sources)
                } else {
                    if (!(this.staticImage && this._multiImage === this._image)) {
                        this._native.multiSetImage(multi, this._image, this._width, this._height);
                        this._multiImage = this._image;
                    }
                    datas = this._native.multiWarpBatch(multi, pts, g);
                }
            } else {
                this._uploadMesh();
                datas = this._batchSources(images, (...src) => this._native.warpInversePiecewiseBatch(this._ctx, pts, g, own, ...src));
            }
            inv.forEach((f, k) => { frames[f] = makeImageData(datas[k], g[4 * k + 2], g[4 * k + 3]); });
        }
        if (fwd.length) {                                                                               // _piecewiseAffineWarp :948-972 for the frames warp() sends there
            const { pts, g, images } = subset(fwd);
            room(g);
            this._uploadMesh();
            const datas = this._batchSources(images, (...src) => this._native.warpForwardPiecewiseBatch(this._ctx, pts, this._maxSrcX, this._maxSrcY, g, own, ...src));
            fwd.forEach((f, k) => { frames[f] = makeImageData(datas[k], g[4 * k + 2], g[4 * k + 3]); });
        }
        for (const { f, map, mats, blank: isBlank } of stale) {                                         // forward frames over a stale map: one by one, as they stand
            if (isBlank) { if (options.images) this._uploadSources([options.images[f % options.images.length]]); else this._uploadImage(); this._forwardOverHeldMap(mats, map, 0, 0, 0, 0); continue; }
            const [xo, yo, ow, oh] = geoms.subarray(4 * f, 4 * f + 4);
            makeRoomFor(this._native, ow * oh * 4, 1);
            if (options.images) this._uploadSources([options.images[f % options.images.length]]); else this._uploadImage();
            frames[f] = makeImageData(this._forwardOverHeldMap(mats, map, xo, yo, ow, oh), ow, oh);
        }
        for (let f = 0; f < F; f++) if (blank[f] === true) frames[f] = makeImageData(new Uint8ClampedArray(4), 1, 1);
        if (F > 0) this._lastPath = forward[F - 1] ? '_piecewiseAffineWarp' : '_inversePiecewiseAffineWarp';   // what the last warp() of the loop leaves behind
        return this._releasable(frames);
    }

    /**
     * The loop `for (f) { setDestinyPoints(dst[f]); warp(image_f, false, true); }` with all frames blended into ONE picture on the device
     * (not part of the reference; include/hgwarp.h, hg_mosaic_frames_device): a panorama, a stack of aligned exposures, a stabilised clip
     * pasted on one canvas.  The frames are warped into device memory (in the instance's sampling mode), their coordinate fields are
     * exported beside them, and only the canvas comes down.  Piecewise, affine and projective transforms.
     *   options.blend     'feather' (default): every frame weighs in by the distance of the pixel's SOURCE position to the border of the
     *                     source image, in source pixels, capped at options.feather -- seams fade; 'mean': plain average of the frames
     *                     that cover the pixel; 'last': the last frame that covers it (painter's order); 'multiband': every pixel is
     *                     owned by the frame with the largest 'feather' weight, and the frames are blended across the seams between
     *                     owners in options.bands frequency bands -- low frequencies over a wide range, so exposure differences fade,
     *                     high frequencies over a narrow one, so detail comes from one frame and nothing is doubled
     *                     (include/hgwarp.h, hg_mosaic_multiband_device; the weight plane is then 1 where a frame owns the pixel);
     *                     'median', 'trimmed', 'min', 'max': an order statistic of the frames that cover the pixel, channel by channel
     *                     (include/hgwarp.h, hg_mosaic_robust_device) -- what moves through a minority of the frames of a stack drops
     *                     out of the median and of the trimmed mean with no mask or threshold; 'min' / 'max' keep the darkest /
     *                     brightest value.  At most 256 non-blank frames; the weight plane is then the number of frames that cover
     *                     the pixel; options.feather and options.bands are ignored; 8-bit images only (an f32 image is a TypeError);
     *   options.trim      'trimmed' only: the share cut off at EACH end before the rest is averaged, a number in [0, 0.5) (default 0.25;
     *                     0: the mean);
     *   options.bands     the band count of 'multiband', an integer 1..8 (default 5; 1: a paste along the seams);
     *   options.labels    'multiband' only, true: also return labels, an Int32Array of the owning destiny point set per canvas pixel
     *                     (-1: none);
     *   options.feather   the cap of the 'feather' weight, a number > 0 (default Infinity: uncapped);
     *   options.canvas    { x, y, width, height } in the windows' coordinate system (four integers); default: the bounding box of the
     *                     non-blank windows;
     *   options.images    the loop warp(image_f): frame f reads images[f % images.length];
     *   options.pointsAreNormalized   the second argument of every setDestinyPoints;
     *   options.weight    true: also return the weight plane (the sum of the weights per canvas pixel; 0 where no frame covers).
     *   options.exposure  equalise the frames' exposures before the blend, one gain per frame on the colour channels, alpha untouched
     *                     (include/hgwarp.h, hg_mosaic_frames_gain_device).  'gain': the gains are fitted on the overlaps (Brown & Lowe's gain
     *                     compensation, sigmaN = 10, sigmaG = 0.1): the overlaps are measured on the device, 16 F^2 bytes come down, a small
     *                     system is solved on the host -- the frames never leave the device; at most 256 non-blank frames.
     *                     { sigmaN, sigmaG }: the same with these parameters (numbers > 0).  An array or Float32Array of one gain per
     *                     destiny point set (finite, > 0): applied as given.  'none' or absent: no gains.  The result then also carries
     *                     `gains`, a Float32Array of one gain per destiny point set (1 for a blank frame).
     * Every setDestinyPoints(dst[f]) runs on the host exactly as in warpBatch(dstPointSets, {inverse: true}), so the instance ends in the
     * state that call leaves.  A pixel no frame covers is 0 in every channel; where exactly one frame covers it, its bytes are that frame's.
     * Returns { data: Uint8ClampedArray, width, height, x, y [, weight: Float32Array] [, labels: Int32Array] }.  Throws a string for an
     * unknown blend, bad `bands`, `labels` without 'multiband', a bad feather, a bad `trim`, a canvas that is not four integers, a bad `exposure`, and for `devices` and `sourcePoints` (the mosaic runs on this
     * instance's own device, over one source point set).
     */
    mosaic(dstPointSets, options = {}) {
        if (options === null || options === undefined) options = {};
        const blend = options.blend === undefined ? 'feather' : options.blend;
        const multiband = blend === 'multiband';
        const robust = ['median', 'trimmed', 'min', 'max'].indexOf(blend);      // HG_ROBUST_*
        const mode = robust >= 0 ? robust : ['last', 'mean', 'feather'].indexOf(blend);
        if (mode < 0 && !multiband) throw ("mosaic: options.blend must be 'feather', 'mean', 'last', 'multiband', 'median', 'trimmed', 'min' or 'max'");
        if (robust >= 0 && typeof this._native.mosaicRobustInverseGeometric !== 'function')      // (an addon from before hg_mosaic_robust_device)
            throw (`mosaic: options.blend '${blend}' needs an addon built with the robust mosaics; this one knows 'feather', 'mean', 'last' and 'multiband'`);
        const trim = options.trim === undefined ? 0.25 : options.trim;
        if (blend === 'trimmed' && !(typeof trim === 'number' && trim >= 0 && trim < 0.5)) throw ("mosaic: options.trim must be a number in [0, 0.5)");
        const bands = options.bands === undefined ? 5 : options.bands;
        if (multiband && !(Number.isInteger(bands) && bands >= 1 && bands <= 8)) throw ("mosaic: options.bands must be an integer 1..8");
        if (!multiband && options.labels === true) throw ("mosaic: options.labels needs blend 'multiband'");
        const wantLabels = multiband && options.labels === true;
        const feather = options.feather === undefined || robust >= 0 ? Infinity : options.feather;
        if (typeof feather !== 'number' || !(feather > 0)) throw ("mosaic: options.feather must be a number > 0 (Infinity: uncapped)");
        let canvas = null;
        if (options.canvas !== undefined && options.canvas !== null) {
            const c = options.canvas;
            canvas = [c.x, c.y, c.width, c.height];
            if (!canvas.every((v) => Number.isInteger(v) && Math.abs(v) <= 0x7fffffff)) throw ("mosaic: options.canvas must be { x, y, width, height }, four integers");
        }
        if (options.devices !== undefined && options.devices !== null) throw ("mosaic: runs on this instance's own device; {devices} is not supported");
        if (options.sourcePoints !== undefined && options.sourcePoints !== null) throw ("mosaic: one source point set for all frames; {sourcePoints} is not supported");
        if (!Array.isArray(dstPointSets)) throw ("mosaic: needs an array of destiny point sets");
        let exposure = null;                                     // null, a Float64Array [sigmaN, sigmaG] (fit the gains) or a Float32Array of F gains
        const ex = options.exposure;
        if (ex !== undefined && ex !== null && ex !== 'none') {
            const bad = "mosaic: options.exposure must be 'gain', 'none', { sigmaN, sigmaG } (numbers > 0) or one finite gain > 0 per destiny point set";
            if (ex === 'gain') exposure = Float64Array.of(10, 0.1);
            else if (Array.isArray(ex) || ex instanceof Float32Array) {
                if (ex.length !== dstPointSets.length || !Array.prototype.every.call(ex, (g) => typeof g === 'number' && Number.isFinite(g) && g > 0)) throw (bad);
                exposure = Float32Array.from(ex);
                if (!exposure.every((g) => Number.isFinite(g) && g > 0)) throw (bad);      // (a double that leaves the float32 range)
            } else if (typeof ex === 'object' && !ArrayBuffer.isView(ex)) {
                const sn = ex.sigmaN === undefined ? 10 : ex.sigmaN, sg = ex.sigmaG === undefined ? 0.1 : ex.sigmaG;
                if (typeof sn !== 'number' || typeof sg !== 'number' || !Number.isFinite(sn) || !Number.isFinite(sg) || !(sn > 0) || !(sg > 0)) throw (bad);
                exposure = Float64Array.of(sn, sg);
            } else throw (bad);
        }
        const geometric = this.transform === 'affine' || this.transform === 'projective';
        if (!geometric && this.transform !== 'piecewiseaffine') throw ("hgwarp: mosaic() needs a transform (set the source points first)");
        const images = options.images === undefined ? null : options.images;
        if (robust >= 0) {                                       // the order statistics rank bytes
            const isF32 = (im) => im instanceof Float32Array || (im !== null && typeof im === 'object' && im.data instanceof Float32Array);
            if ((Array.isArray(images) && images.some(isF32)) || (!images && isF32(this._image))) throw new TypeError(`mosaic: blend '${blend}' takes 8-bit images only`);
        }
        const F = dstPointSets.length, n = geometric ? (this.transform === 'affine' ? 6 : 8) : this._srcPoints.length;
        const dsts = new Float32Array(F * n), srcPts = new Float32Array(geometric ? F * n : 0), geoms = new Int32Array(F * 4), keep = [];
        for (let f = 0; f < F; f++) {                            // warpBatch(dstPointSets, {inverse: true})'s host loop, frame for frame
            this.setDestinyPoints(dstPointSets[f], options.pointsAreNormalized === undefined ? null : options.pointsAreNormalized);
            if (this._image === null && !images) throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");
            const [xo, yo, ow, oh] = this._window();
            if (geometric) {
                this._alignRanges();                                                                     // :993
                dsts.set(asF32(this._dstPoints).subarray(0, n), f * n);                                    // inverse: dst -> src (:994)
                srcPts.set(asF32(this._srcPoints).subarray(0, n), f * n);
            } else {
                dsts.set(asF32(this._dstPoints), f * n);
                checkedMapLength(ow * oh);
                this._map = { kind: 'inverse', pts: dsts.subarray(f * n, (f + 1) * n), tris: this._triangles, width: ow, height: oh, yOff: yo };
            }
            if (!(ow * oh >= 1)) continue;                                                               // :440: a blank frame covers nothing
            checkedLength(ow * oh * 4);
            geoms.set([xo, yo, ow, oh], f * 4);
            keep.push(f);
        }
        if (F > 0) this._lastPath = geometric ? '_inverseGeometricWarp' : '_inversePiecewiseAffineWarp';
        if (canvas === null) {
            let x0 = Infinity, y0 = Infinity, x1 = -Infinity, y1 = -Infinity;
            for (const f of keep) {
                x0 = Math.min(x0, geoms[4 * f]); y0 = Math.min(y0, geoms[4 * f + 1]);
                x1 = Math.max(x1, geoms[4 * f] + geoms[4 * f + 2]); y1 = Math.max(y1, geoms[4 * f + 1] + geoms[4 * f + 3]);
            }
            canvas = keep.length ? [x0, y0, x1 - x0, y1 - y0] : [0, 0, 0, 0];
        }
        const [cx, cy] = canvas, cw = Math.max(canvas[2], 0), ch = Math.max(canvas[3], 0);
        const out = { data: null, width: cw, height: ch, x: cx, y: cy };
        checkedLength(cw * ch * 4);
        if (keep.length === 0 || cw * ch === 0) {                // nothing to blend: the zero canvas
            out.data = new Uint8ClampedArray(cw * ch * 4);
            if (options.weight === true) out.weight = new Float32Array(cw * ch);
            if (wantLabels) out.labels = new Int32Array(cw * ch).fill(-1);
            if (exposure !== null) out.gains = exposure instanceof Float32Array ? exposure : new Float32Array(F).fill(1);
            return out;
        }
        const sub = (arr, w) => { if (keep.length === F) return arr; const o = new arr.constructor(keep.length * w); keep.forEach((f, k) => o.set(arr.subarray(f * w, (f + 1) * w), k * w)); return o; };
        const tail = [multiband ? bands : mode, robust >= 0 ? (blend === 'trimmed' ? trim : 0) : feather, Int32Array.from([cx, cy, cw, ch]), options.weight === true, this._width, this._height];
        if (multiband) tail.push(wantLabels);
        if (exposure !== null) tail.push(exposure instanceof Float32Array ? sub(exposure, 1) : exposure);      // (absent: the call is what it was)
        const srcs = images === null ? null : keep.map((f) => images[f % images.length]);
        let res;
        if (geometric) {
            this._uploadSources(srcs);
            res = this._native[multiband ? 'mosaicMultibandInverseGeometric' : robust >= 0 ? 'mosaicRobustInverseGeometric' : 'mosaicInverseGeometric'](this._ctx, this.transform === 'affine' ? AFFINE : PROJECTIVE, sub(dsts, n), sub(srcPts, n), sub(geoms, 4), ...tail);
        } else {
            this._uploadMesh();
            this._uploadSources(srcs);
            res = this._native[multiband ? 'mosaicMultibandInversePiecewise' : robust >= 0 ? 'mosaicRobustInversePiecewise' : 'mosaicInversePiecewise'](this._ctx, sub(dsts, n), sub(geoms, 4), ...tail);
        }
        out.data = res.data;
        if (options.weight === true) out.weight = res.weight;
        if (wantLabels) out.labels = keep.length === F ? res.labels : res.labels.map((l) => (l < 0 ? l : keep[l]));      // (the blank frames were not part of the call)
        if (exposure !== null) {                                 // one gain per destiny point set: the blank frames were not part of the call
            out.gains = new Float32Array(F).fill(1);
            keep.forEach((f, k) => { out.gains[f] = res.gains[k]; });
        }
        return out;
    }

    /**
     * warpBatch(dst, {sourcePoints: src}): the loop `setSourcePoints(src[f]); setDestinyPoints(dst[f]); warp(image_f)`, frame for frame.  Both
     * setters run on the host exactly as in the loop, so every frame sees the instance as the loop would have left it: the source points of
     * the moment, `_minSrcX / _minSrcY` AS THEY STAND (the reference refreshes them only while its map field is null, :252, :756-758: after
     * the first frame they are stale, and the stale values are what :1047 tests), the window, and warp()'s dispatch (:421-422).  Frames
     * that take the inverse loop with current matrices are recorded and go out as ONE batch through warpInversePiecewiseSrcBatch
     * (hg_warp_inverse_piecewise_src_batch_device: per-frame source points and minima; own or pooled frames, {images} pipelined).  Every
     * other frame -- the forward loop, a warp over held (stale) matrices, a blank window -- runs at once through warp() itself, in its
     * place in the order.  Bare strings: a source list of another length, a transform that is not piecewise, {devices}.
     */
    _warpBatchMoving(dstPointSets, options) {
        const srcSets = options.sourcePoints, F = dstPointSets.length;
        if (this.transform !== 'piecewiseaffine' && this.firstTransformSelected !== 'piecewiseaffine')
            throw (`hgwarp: warpBatch({sourcePoints}) needs a piecewise affine transform, but ${this.transform} is selected`);
        if (!Array.isArray(srcSets) || srcSets.length !== F)
            throw (`hgwarp: warpBatch({sourcePoints}) needs one source point set per destiny point set (${Array.isArray(srcSets) ? srcSets.length : 'none'} for ${F})`);
        if (options.devices !== undefined && options.devices !== null)
            throw ("hgwarp: warpBatch({sourcePoints}) runs on this instance's own device; {devices} cannot be combined with it");
        const images = options.images === undefined || options.images === null ? null : options.images;
        if (images !== null && (!Array.isArray(images) || images.length === 0)) throw ("hgwarp: warpBatch({images}) needs a non-empty array of ImageData-shaped sources");
        const frames = new Array(F).fill(null);
        const reuse = !(options.ownFrames === true || !(options.reuseBatchOutput === undefined ? this.reuseBatchOutput : options.reuseBatchOutput === true));
        let pending = [], flushed = 0;
        const flush = (last) => {
            if (pending.length === 0) return;
            const K = pending.length, n = pending[0].src.length;
            const src = new Float32Array(K * n), dst = new Float32Array(K * n), mins = new Int32Array(K * 2), g = new Int32Array(K * 4);
            pending.forEach((p, k) => { src.set(p.src, k * n); dst.set(p.dst, k * n); mins.set(p.min, 2 * k); g.set(p.win, 4 * k); });
            // (the instance's one slab serves one native batch: only a batch that is both the first and the last of this call may use it)
            const own = !(reuse && last && flushed === 0);
            if (own) { let largest = 0; for (const p of pending) largest = Math.max(largest, p.win[2] * p.win[3] * 4); makeRoomFor(this._native, largest, K); }
            const tris = pending[0].tris instanceof Uint32Array ? pending[0].tris : Uint32Array.from(pending[0].tris);
            this._native.piecewiseSetMesh(this._ctx, pending[0].src, tris, pending[0].min[0], pending[0].min[1]);   // triangles + point count; the source side travels per frame
            let datas;
            if (images === null) { this._uploadImage(); datas = this._native.warpInversePiecewiseSrcBatch(this._ctx, src, mins, dst, g, own); }
            else {                                                                                       // (the native side pipelines the uploads with the downloads)
                datas = this._native.warpInversePiecewiseSrcBatch(this._ctx, src, mins, dst, g, own, pending.map((p) => p.image.data), pending[0].W, pending[0].H);
                this._uploadedImage = null;                                                              // the next single-image warp uploads again
            }
            pending.forEach((p, k) => { frames[p.f] = makeImageData(datas[k], p.win[2], p.win[3]); });
            pending = []; flushed++;
        };
        const i32 = (v) => Number.isInteger(v) && Math.abs(v) < 2147483648;
        for (let f = 0; f < F; f++) {
            this.setSourcePoints(srcSets[f]);                                                            // :218-265, as the loop does
            this.setDestinyPoints(dstPointSets[f], options.pointsAreNormalized === undefined ? null : options.pointsAreNormalized);   // :337-380
            const image = images ? images[f % images.length] : null;
            if (image !== null) this.setImage(image);                                                    // warp(image_f) :409
            else if (this._image === null) throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");
            const [xo, yo, ow, oh] = this._window();
            const inverse = options.inverse === true || this._sampling === 'bilinear' || ow > this._width || oh > this._height || ow * 1.2 < this._width || oh * 1.2 < this._height;   // :421-422
            const batchable = this.transform === 'piecewiseaffine' && inverse && ow * oh >= 1 && (this.repairStaleMap || this._matricesAreCurrent()) &&
                              i32(this._minSrcX) && i32(this._minSrcY) && ow * oh * 4 <= 2147483647;
            if (!batchable) { frames[f] = this.warp(null, false, options.inverse === true); continue; }
            // what _inversePiecewise leaves behind (:847-857)
            this._lastPath = '_inversePiecewiseAffineWarp';
            this._map = { kind: 'inverse', pts: Float32Array.from(this._dstPoints), tris: this._triangles, width: ow, height: oh, yOff: yo };
            // one native batch has one triangle list and one source size
            if (pending.length && !(sameTriangles(pending[0].tris, this._triangles) && pending[0].src.length === this._srcPoints.length &&
                                    pending[0].W === this._width && pending[0].H === this._height)) flush(false);
            pending.push({ f, src: Float32Array.from(this._srcPoints), dst: Float32Array.from(this._dstPoints), min: [this._minSrcX, this._minSrcY],
                           win: [xo, yo, ow, oh], tris: this._triangles, image, W: this._width, H: this._height });
        }
        flush(true);
        return this._releasable(frames);
    }

    /**
     * warpBatch() for affine / projective: every `setDestinyPoints(dst_f)` of the loop runs on the host exactly as in the loop
     * (normalisation auto-detect, in-place range alignment, forward matrix, output window).  Frames that warp() sends down the inverse
     * loop (projective always :431; affine when the output size differs from the source's :426, or with {inverse: true}): the inverse
     * matrices the reference re-solves inside every warp (:994) are solved on the GPU, one lane per frame, all frames in one launch.
     * Affine frames of the source's size go through the forward loop _geometricWarp (:427) with their forward matrices, as one batch.
     */
    _warpBatchGeometric(dstPointSets, options = {}) {
        const F = dstPointSets.length, per = this.transform === 'affine' ? 6 : 8;
        const from = new Float32Array(F * per), to = new Float32Array(F * per), geoms = new Int32Array(F * 4), mats = new Float64Array(F * 8);
        const blank = new Array(F).fill(false), forward = new Array(F).fill(false);
        for (let f = 0; f < F; f++) {
            this.setDestinyPoints(dstPointSets[f], options.pointsAreNormalized === undefined ? null : options.pointsAreNormalized);
            if (this._image === null && !options.images) throw ("warp() must receive an image if it was not setted before through `setImage(img)` or  `setSourcePoints(points, img)`");   // the loop's first warp() (:411-413)
            const [xo, yo, ow, oh] = this._window();
            forward[f] = this.transform === 'affine' && options.inverse !== true && this._sampling !== 'bilinear' && ow === this._width && oh === this._height;      // :426-427, :431
            if (forward[f]) mats.set(Array.from(this._transformMatrix), f * 8);                          // _geometricWarp uses _transformMatrix as it stands (:915)
            else {
                this._alignRanges();                                                                     // :993
                from.set(asF32(this._dstPoints).subarray(0, per), f * per);                              // inverse: dst -> src (:994)
                to.set(asF32(this._srcPoints).subarray(0, per), f * per);
            }
            if (!(ow * oh >= 1)) { blank[f] = true; geoms.set([0, 0, 0, 0], f * 4); continue; }
            checkedLength(ow * oh * 4);
            geoms.set([xo, yo, ow, oh], f * 4);
        }
        const kind = this.transform === 'affine' ? AFFINE : PROJECTIVE;
        const frames = new Array(F).fill(null);
        const pick = (want) => { const ids = []; for (let f = 0; f < F; f++) if (!blank[f] && forward[f] === want) ids.push(f); return ids; };
        const own = options.ownFrames === true || !(options.reuseBatchOutput === undefined ? this.reuseBatchOutput : options.reuseBatchOutput === true);
        const room = (g) => { if (!own) return; let largest = 0; for (let k = 0; k < g.length / 4; k++) largest = Math.max(largest, g[4 * k + 2] * g[4 * k + 3] * 4); makeRoomFor(this._native, largest, g.length / 4); };
        const sub = (arr, ids, w) => { if (ids.length === F) return arr; const o = new arr.constructor(ids.length * w); ids.forEach((f, k) => o.set(arr.subarray(f * w, (f + 1) * w), k * w)); return o; };
        const subImages = (ids) => (options.images && ids.length !== F ? ids.map((f) => options.images[f % options.images.length]) : options.images);
        const inv = pick(false), fwd = pick(true);
        if (inv.length) {
            const g = sub(geoms, inv, 4), fr = sub(from, inv, per), tt = sub(to, inv, per), images = subImages(inv);
            room(g);
            let datas;
            if (options.devices !== undefined && options.devices !== null) {                          // frames spread over several GPUs
                const multi = this._multiFor(options.devices);
                if (images) {
                    datas = this._native.multiWarpGeometricBatch(multi, kind, fr, tt, g, this._checkedSources(images), this._width, this._height);
                    this._multiImage = null;
                } else {
                    if (!(this.staticImage && this._multiImage === this._image)) {
                        this._native.multiSetImage(multi, this._image, this._width, this._height);
                        this._multiImage = this._image;
                    }
                    datas = this._native.multiWarpGeometricBatch(multi, kind, fr, tt, g);
                }
            } else {
                datas = this._batchSources(images, (...src) => this._native.warpInverseGeometricBatch(this._ctx, kind, fr, tt, g, own, ...src));
            }
            inv.forEach((f, k) => { frames[f] = makeImageData(datas[k], g[4 * k + 2], g[4 * k + 3]); });
        }
        if (fwd.length) {                                                                               // _geometricWarp :911-932
            const g = sub(geoms, fwd, 4), m = sub(mats, fwd, 8);
            room(g);
            const datas = this._batchSources(subImages(fwd), (...src) => this._native.warpForwardGeometricBatch(this._ctx, kind, m, g, own, ...src));
            fwd.forEach((f, k) => { frames[f] = makeImageData(datas[k], g[4 * k + 2], g[4 * k + 3]); });
        }
        for (let f = 0; f < F; f++) if (blank[f]) frames[f] = makeImageData(new Uint8ClampedArray(4), 1, 1);
        if (F > 0) this._lastPath = forward[F - 1] ? '_geometricWarp' : '_inverseGeometricWarp';
        return this._releasable(frames);
    }

    /** hg_multi handle for a device list (kept while the list stays the same). */
    _multiFor(devices) {
        const ids = Int32Array.from(devices);
        if (ids.length === 0) throw ("hgwarp: warpBatch({devices}) needs at least one device id");
        const key = ids.join(',');
        if (this._multiKey !== key) {
            if (this._multiHandle) this._native.multiDestroy(this._multiHandle);
            this._multiHandle = this._native.multiCreate(ids);
            this._multiKey = key; this._multiImage = null;
            if (this._sampling !== 'nearest') this._native.multiSetSampling(this._multiHandle, SAMPLING.indexOf(this._sampling));
        }
        return this._multiHandle;
    }

    getTransformationMatrixAsCSS(srcPoints = null, dstPoints = null, width = null, height = null) {     // :548-587
        if (width !== null || height !== null) this._setSourceSize(width, height);
        if (srcPoints !== null) this.setSourcePoints(srcPoints, null, width, height);
        if (dstPoints !== null) this.setDestinyPoints(dstPoints);
        if (this._srcPoints === null) throw ("Impossible to calculate a transform when srcPoints are not set");
        else if (this._dstPoints === null) throw ("Impossible to calculate a transform when dstPoints are not set");
        else if (this._transformMatrix === null) throw ("Transform matrix can not be calculated");
        const m = this._transformMatrix, fx = (v) => v.toFixed(CSS_DECIMALS);
        if (this.transform === 'affine') return `matrix(${Array.from(m, fx).join(', ')})`;
        if (this.transform === 'projective') {
            const cells = [];
            let i = 0;
            for (let row = 0; row < 4; row++) for (let col = 0; col < 4; col++) {
                if ((row === 2 && col === 2) || (row === 3 && col === 3)) cells.push('1');
                else if (row === 2 || col === 2) cells.push('0');
                else cells.push(fx(m[((i++) * 3) % 8]));
            }
            return `matrix3d(${cells.join(', ')})`;
        }
        throw (`Only "affine" or "projective" transforms can be applied on the CSS transform property, but ${this.transform} selected`);
    }

    HTMLImageElementFromImageData() { throw ("hgwarp: HTMLImageElementFromImageData() needs a browser DOM"); }
    transformHTMLElement() { throw ("hgwarp: transformHTMLElement() needs a browser DOM"); }

    // ------------------------------------------------------------------------------------------------ parity taps (debug)
    /** Int16Array the reference's _buildInverseTrianglesCorrespondencesMatrix would hold for the last inverse piecewise warp. */
    triangleMap(fused = true) { return this._native.getTriMap(this._ctx, !!fused); }
    /** {forward, inverse}: per-triangle Float32Array(6 T) of the last piecewise warp. */
    piecewiseMatrices() { return this._native.getMatrices(this._ctx, this._triangles.length / 3); }

    // ------------------------------------------------------------------------------------------------ private
    _solve(from, to) {                                                                                   // :1237-1250
        // a point set shorter than the transform needs (an 'auto' instance between a 4-point setSourcePoints and the matching
        // setDestinyPoints): the reference reads `undefined` past the end, i.e. NaN in its arithmetic
        const need = this.transform === 'affine' ? 6 : 8;
        const padded = (p) => { p = asF32(p); if (p.length >= need) return p; const q = new Float32Array(need).fill(NaN); q.set(p); return q; };
        const a = padded(from), b = padded(to);
        if (this.transform === 'affine') return this._native.solveAffine(a, b);                          // Float32Array(6)
        if (this.transform === 'projective') return Array.from(this._native.solveProjective(a, b));      // plain Array(8) of doubles, as numeric.js returns
        throw (`${this.transform} transform does not exist`);
    }

    _setSourceSize(width, height) {                                                                      // :637-679
        const lastW = this._width, lastH = this._height;
        this._width = width; this._height = height;
        if (lastW === width && lastH === height) return;
        this._width = Math.round(width); this._height = Math.round(height);
        this._map = null;                                                                                // :647
        if (this.transform === 'projective') {
            if (this._srcPoints !== null && this._srcPointsAreNormalized) { scalePoints(this._srcPoints, this._width, this._height); this._srcPointsAreNormalized = false; }
            if (this._dstPoints !== null && this._dstPointsAreNormalized) { scalePoints(this._dstPoints, this._width, this._height); this._dstPointsAreNormalized = false; }
            if (this._dstPoints !== null && this._srcPoints !== null) {
                this._transformMatrix = this._solve(this._srcPoints, this._dstPoints);
                this._deriveOutputWindow();
            }
        }
        if (this._srcPoints !== null && this.transform === 'piecewiseaffine') this._refreshPiecewise();
    }

    _deriveOutputWindow() {                                                                              // :693-725
        if (this.transform === 'affine' || this.transform === 'projective') {
            if (this._transformMatrix === null) {
                if (this._srcPointsAreNormalized !== this._dstPointsAreNormalized) this._alignRanges();
                this._transformMatrix = this._solve(this._srcPoints, this._dstPoints);
            }
            const lim = this._native.transformLimits(this.transform === 'affine' ? AFFINE : PROJECTIVE, Float64Array.from(this._transformMatrix), this._width, this._height);
            [this._xOutputOffset, this._yOutputOffset, this._objectiveWidth, this._objectiveHeight] = lim;
        } else if (!this._dstPointsAreNormalized) {
            const mm = this._native.minmaxXY(asF32(this._dstPoints));                                    // rounded min/max, then subtract (:707-710)
            this._xOutputOffset = mm[0]; this._yOutputOffset = mm[1];
            this._objectiveWidth = mm[2] - mm[0]; this._objectiveHeight = mm[3] - mm[1];
        } else if (this._width > 0 && this._height > 0) {
            let minX = Infinity, minY = Infinity, maxX = -Infinity, maxY = -Infinity;                    // unrounded (:714-718)
            const p = this._dstPoints;
            for (let i = 0; i < p.length; i++) {
                if ((i % 2) === 0) { if (p[i] > maxX) maxX = p[i]; if (p[i] < minX) minX = p[i]; }
                else { if (p[i] > maxY) maxY = p[i]; if (p[i] < minY) minY = p[i]; }
            }
            this._xOutputOffset = Math.round(minX); this._yOutputOffset = Math.round(minY);
            this._objectiveWidth = Math.round((maxX - minX) * this._width);
            this._objectiveHeight = Math.round((maxY - minY) * this._height);
        } else {
            throw ("Trying to calculate a the output width and height of a Piecewise Affine transform but source width and height are not set");
        }
    }

    _refreshPiecewise() {                                                                                // :738-774
        if (this._srcPoints === null) throw ("Trying to set the Piecewise Affine Transform parameters before setting the Source Points.");
        if (this._triangles === null) this._triangles = Homography.triangulate(this._srcPoints);
        if (this._srcPointsAreNormalized) {
            if (this._width > 0 && this._height > 0) { scalePoints(this._srcPoints, this._width, this._height); this._srcPointsAreNormalized = false; }
            else throw ("Trying to set the Piecewise Affine Transform parameters without knowing the source points ranges");
        }
        if (!this._srcPointsAreNormalized && (this._triangles === null || this._map === null)) {
            const mm = this._native.minmaxXY(asF32(this._srcPoints));                                    // :758
            [this._minSrcX, this._minSrcY, this._maxSrcX, this._maxSrcY] = mm;
            this._snapshotForwardMap();                                                                  // :759
        }
        if (this._dstPoints !== null && this._pm === null && this._triangles !== null) {
            if (this._dstPointsAreNormalized) { scalePoints(this._dstPoints, this._width, this._height); this._dstPointsAreNormalized = false; }
            if (this._srcPointsAreNormalized !== this._dstPointsAreNormalized) this._alignRanges();     // :787-789
            // :769: matrices of THESE point sets (the per-triangle solves run on the GPU with the warp)
            this._pm = { src: Float32Array.from(this._srcPoints), dst: Float32Array.from(this._dstPoints), tris: this._triangles };
        }
    }

    _alignRanges() {                                                                                     // :876-896
        if (this._dstPointsAreNormalized === this._srcPointsAreNormalized) return;
        if (this._dstPointsAreNormalized && this._width > 0 && this._height > 0) {
            unscalePoints(this._srcPoints, this._width, this._height);
            this._srcPointsAreNormalized = true;
        } else if (this._srcPointsAreNormalized && this._width > 0 && this._height > 0) {
            scalePoints(this._srcPoints, this._width, this._height);
            this._srcPointsAreNormalized = false;
        } else {
            throw ("Impossible to put source and destiny points in the same range. Possible solutions: \n" +
                   "1. Give a source width/height when calling setSrcPoints.\n" +
                   "2. Set the input image before.\n" +
                   "3. Give Source and Destiny points in the same range (both normalized or both in image dimensions)");
        }
    }

    _uploadImage() {
        // The reference re-reads the caller's buffer on every warp (:298), so a mutated buffer must show up: upload every time
        // (unless the caller opted into `staticImage`).
        const ctx = this._ctx;
        if (this.staticImage && this._uploadedImage === this._image && this._uploadedCtx === ctx) return;
        this._native.setImage(ctx, this._image, this._width, this._height);
        this._uploadedImage = this._image; this._uploadedCtx = ctx;
    }

    /** Source(s) of a batch: the instance's image, or `images` (one ImageData-shaped source per frame, all of the instance's size:
     *  the loop `warp(image_f)`; frame f reads images[f % images.length]). */
    _checkedSources(images) {
        if (!Array.isArray(images) || images.length === 0) throw ("hgwarp: warpBatch({images}) needs a non-empty array of ImageData-shaped sources");
        for (const im of images) {
            if (!im || !ArrayBuffer.isView(im.data) || im.width !== this._width || im.height !== this._height)
                throw ("hgwarp: every image of warpBatch({images}) must be ImageData-shaped and of the size the instance was set up with");
        }
        return images.map((im) => im.data);
    }

    _uploadSources(images) {
        if (images === undefined || images === null) return this._uploadImage();
        this._native.setImages(this._ctx, this._checkedSources(images), this._width, this._height);
        this._uploadedImage = null;                              // the next single-image warp uploads again
    }

    /** Runs a native batch with the instance's image (uploaded first) or with per-frame sources handed to the native side, which
     *  pipelines their uploads with the downloads of the frames (frame f reads images[f % images.length]). */
    _batchSources(images, run) {
        if (images === undefined || images === null) { this._uploadImage(); return run(); }
        const datas = run(this._checkedSources(images), this._width, this._height);
        this._uploadedImage = null;                              // the next single-image warp uploads again
        return datas;
    }

    /** The frames of a batch + `release()`: the page-locked buffer behind them goes back at once (they become empty). */
    _releasable(frames) {
        Object.defineProperty(frames, 'release', { value: () => { if (this._ctxHandle) this._native.releaseBatch(this._ctxHandle); }, enumerable: false });
        return frames;
    }

    _uploadMesh() {
        const tris = this._triangles instanceof Uint32Array ? this._triangles : Uint32Array.from(this._triangles);
        this._native.piecewiseSetMesh(this._ctx, asF32(this._srcPoints), tris, this._minSrcX, this._minSrcY);
    }

    _window() { return [this._xOutputOffset, this._yOutputOffset, this._objectiveWidth, this._objectiveHeight]; }

    /** The caller-owned output buffer handed to the addon when `reuseOutput` is on (grown as needed), else undefined. */
    _reusable(bytes) {
        if (!this.reuseOutput) return undefined;
        if (this._outBuffer === null || this._outBuffer.length < bytes) this._outBuffer = new Uint8ClampedArray(bytes);
        return this._outBuffer;
    }

    _inverseGeometric() {                                                                                // :987-1013
        this._lastPath = '_inverseGeometricWarp';
        this._alignRanges();
        const inv = this._solve(this._dstPoints, this._srcPoints);                                       // re-solved from the swapped sets (:994)
        this._uploadImage();
        const [xo, yo, ow, oh] = this._window();
        if (!(ow * oh >= 1)) return new Uint8ClampedArray(0);
        checkedLength(ow * oh * 4);
        if (!this.reuseOutput) makeRoomFor(this._native, ow * oh * 4, 1);
        return this._native.warpInverseGeometric(this._ctx, this.transform === 'affine' ? AFFINE : PROJECTIVE, Float64Array.from(inv), xo, yo, ow, oh,
                                                 this._reusable(ow * oh * 4));
    }

    /** Do the cached per-triangle matrices (:769) belong to the current point sets and triangles?  (Always, unless source points or
     *  triangles were replaced after the last setDestinyPoints: :252-255, :519.) */
    _matricesAreCurrent() {
        const pm = this._pm;
        return pm !== null && sameTriangles(pm.tris, this._triangles) && samePoints(pm.src, this._srcPoints) && samePoints(pm.dst, this._dstPoints);
    }

    /** Does the shared map field hold the forward map of the current mesh (:817-832 over the current source bbox)? */
    _mapIsCurrentForward() {
        const m = this._map;
        return m !== null && m.kind === 'forward' && m.width === this._maxSrcX - this._minSrcX && m.height === this._maxSrcY - this._minSrcY &&
               m.yOff === this._minSrcY && sameTriangles(m.tris, this._triangles) && samePoints(m.pts, this._srcPoints);
    }

    /** Forward matrices of the snapshot the reference's `_piecewiseMatrices` came from, 6 floats per triangle (host-side solves). */
    _snapshotMatrices() {
        const pm = this._pm;
        if (pm === null) throw new TypeError("Cannot read property 'length' of null");                  // this._piecewiseMatrices.length (:1036) / [inTriangle] (:961)
        const tris = pm.tris instanceof Uint32Array ? pm.tris : Uint32Array.from(pm.tris);
        return this._native.solveAffineTriangles(pm.src, pm.dst, tris);
    }

    _inversePiecewise() {                                                                                // :1029-1058
        this._lastPath = '_inversePiecewiseAffineWarp';
        const [xo, yo, ow, oh] = this._window();
        checkedMapLength(ow * oh);                                                                       // :848
        // :847-857: the shared field now holds the INVERSE map of these destiny points over this window
        this._map = { kind: 'inverse', pts: Float32Array.from(this._dstPoints), tris: this._triangles, width: ow, height: oh, yOff: yo };
        const current = this.repairStaleMap || this._matricesAreCurrent();
        const mats = current ? null : this._snapshotMatrices();
        if (!(ow * oh >= 1)) return new Uint8ClampedArray(0);
        checkedLength(ow * oh * 4);
        this._uploadImage();
        if (!this.reuseOutput) makeRoomFor(this._native, ow * oh * 4, 1);
        if (!current) {
            // matrices of an OLDER point set / triangle list over the map of the current one (setSourcePoints or setTriangles without a
            // setDestinyPoints since): the reference's loop as it stands, through the materialised map
            const tris = this._triangles instanceof Uint32Array ? this._triangles : Uint32Array.from(this._triangles);
            return this._native.warpInversePiecewiseState(this._ctx, mats, asF32(this._dstPoints), tris, this._minSrcX, this._minSrcY, xo, yo, ow, oh);
        }
        this._uploadMesh();
        this._native.piecewisePrepare(this._ctx, asF32(this._dstPoints), xo, yo, ow, oh);
        return this._native.warpInversePiecewise(this._ctx, this._reusable(ow * oh * 4));
    }

    _forwardGeometric() {                                                                                // :911-932
        this._lastPath = '_geometricWarp';
        this._uploadImage();
        const [xo, yo, ow, oh] = this._window();
        if (!(ow * oh >= 1)) return new Uint8ClampedArray(0);
        checkedLength(ow * oh * 4);
        makeRoomFor(this._native, ow * oh * 4, 1);
        return this._native.warpForwardGeometric(this._ctx, this.transform === 'affine' ? AFFINE : PROJECTIVE, Float64Array.from(this._transformMatrix), xo, yo, ow, oh);
    }

    _forwardPiecewise() {                                                                                // :948-972
        this._lastPath = '_piecewiseAffineWarp';
        const [xo, yo, ow, oh] = this._window();
        const usual = this.repairStaleMap || (this._mapIsCurrentForward() && this._matricesAreCurrent());
        const map = this._map, mats = usual ? null : this._snapshotMatrices();
        if (!usual && map === null) throw new TypeError("Cannot read property '0' of null");              // :957 on a null map
        if (this.repairStaleMap && !this._mapIsCurrentForward()) this._snapshotForwardMap();
        this._uploadImage();
        if (!(ow * oh >= 1)) {
            // a blank window (:440) does not stop the reference's loop: it walks the source bbox over the held map and throws where a
            // cell names a matrix that does not exist -- the stale state still gets that check
            if (!usual) this._forwardOverHeldMap(mats, map, 0, 0, 0, 0);
            return new Uint8ClampedArray(0);
        }
        checkedLength(ow * oh * 4);
        makeRoomFor(this._native, ow * oh * 4, 1);
        if (!usual) {
            // :957 reads whatever the shared field holds -- after an inverse warp the stale INVERSE map of that warp's destiny points,
            // laid out objectiveWidth cells per row but indexed (maxSrcX - minSrcX) per row, cells past its end `undefined` -- and :961
            // the matrices as last solved: both handed over as they stand
            return this._forwardOverHeldMap(mats, map, xo, yo, ow, oh);
        }
        this._uploadMesh();
        return this._native.warpForwardPiecewise(this._ctx, asF32(this._dstPoints), this._maxSrcX, this._maxSrcY, xo, yo, ow, oh);
    }

    /** _piecewiseAffineWarp :948-972 over the map snapshot `map` (whatever the shared field held) with the matrices `mats` as last solved. */
    _forwardOverHeldMap(mats, map, xo, yo, ow, oh) {
        const tris = map.tris instanceof Uint32Array ? map.tris : Uint32Array.from(map.tris);
        // (`new Int16Array(w * h)` of a window that did not exist yet -- null, NaN -- is an empty array: every read is `undefined`)
        const held = map.width * map.height >= 1 ? [map.width, map.height, map.yOff] : [0, 0, 0];
        return this._native.warpForwardPiecewiseState(this._ctx, mats, map.pts, tris, held[0], held[1], held[2],
                                                      this._minSrcX, this._minSrcY, this._maxSrcX, this._maxSrcY, xo, yo, ow, oh);
    }

    /** :759 / :817-832: the shared field becomes the forward map of the CURRENT source points over the current source bbox (built on
     *  the GPU when a forward warp needs it). */
    _snapshotForwardMap() {
        const mw = this._maxSrcX - this._minSrcX, mh = this._maxSrcY - this._minSrcY;
        checkedMapLength(mw * mh);
        this._map = { kind: 'forward', pts: Float32Array.from(this._srcPoints), tris: this._triangles, width: mw, height: mh, yOff: this._minSrcY };
    }
}

function selectTransform(transform, points) {                                                            // :1444-1481
    switch (transform) {
        case 'auto':
            if (points.length === 6) return 'affine';
            if (points.length === 8) return 'projective';
            if (points.length > 8) return 'piecewiseaffine';
            throw (`Transforms must contain at least 3 points but only ${points.length / 2} were given`);
        case 'piecewiseaffine':
            if (points.length < 6) throw (`A piecewise (or affine) transform needs to determine least three reference points but only ${points.length / 2} were given`);
            return transform;
        case 'affine':
            if (points.length !== 6) throw (`An affine transform needs to determine exactly three reference points but ${points.length / 2} were given`);
            return transform;
        case 'projective':
            if (points.length !== 8) throw (`A projective transform needs to determine exactly four reference points but ${points.length / 2} were given`);
            return transform;
        default:
            throw (`Transform "${transform}" is unknown`);
    }
}

/** Triangulator used where the reference calls `new Delaunator(points).triangles` (:1216-1218).  Replaceable. */
Homography.triangulate = defaultTriangulate;
/** Optional: hands the pooled page-locked buffer of a frame returned by warp() / warpBatch() back at once (its data becomes
 *  empty).  Without it the buffer returns when the frame is garbage-collected. */
Homography.release = (imageData) => addon().release(imageData && imageData.data ? imageData.data : imageData);
/** An ImageData-shaped, zero-filled SOURCE image whose pixels live in page-locked memory (to be filled by the caller: decoded video frames
 *  ...): uploads out of it are asynchronous DMA at the full PCIe rate -- with warpBatch({images}) the upload of source f + 1 then really
 *  overlaps the download of frame f.  Images in ordinary V8 memory work everywhere too (the runtime stages them: ~20 % slower uploads). */
Homography.pinnedImage = (width, height) => makeImageData(addon().pinnedBuffer(width * height * 4), width, height);
/** Cap of the page-locked frame pool in bytes (default 2 GiB; 0: plain V8 arrays only).  Returns the bytes currently pinned. */
Homography.setPinnedLimit = (bytes) => addon().setPinnedLimit(bytes);
Homography.poolStats = () => addon().poolStats();
/** GPUs visible to the library. */
Homography.deviceCount = () => addon().deviceCount();
Homography.availableTransforms = TRANSFORMS;

export { Homography };
