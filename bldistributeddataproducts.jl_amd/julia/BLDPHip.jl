#=
BLDPHip.jl — the Julia side of the drop-in: `ccall` bindings to libbldp_hip
(include/bldp.h) for BLDistributedDataProducts.jl's WorkerFunctions.

UNTESTED HERE: Julia is absent from both the build container and the MI355X
box (probed), so this file is the binding a maintainer adds, exercised in this
repo only through the identical Python ctypes binding (_lib.py / tests/).
See INTEGRATION.md for the two-line patch to src/gbtworkerfunctions.jl.
=#
module BLDPHip

using Statistics: mean, median, var, std

export gpu_init, gpu_finalize, gpu_pin, gpu_unpin, gpu_fqav, gpu_reduce, gpu_kurtosis, gpu_band,
       gpu_tstat, gpu_argext, gpu_skewness, gpu_moments, gpu_comm_id, gpu_comm_init, gpu_comm_destroy, gpu_band_gather,
       mad, quantile, gpu_quantile, gpu_quantile_plan, gpu_band_quantile,
       gpu_quantiles, gpu_quantiles_plan, gpu_band_quantiles,
       gpu_outliers, gpu_outliers_plan, gpu_band_outliers,
       gpu_masked_reduce, gpu_band_masked_reduce, gpu_hits, gpu_band_hits,
       gpu_histogram, gpu_histogram_plan, gpu_band_histogram,
       gpu_fold, gpu_fold_plan, gpu_band_fold, gpu_unfold, gpu_band_unfold,
       gpu_dedoppler, gpu_dedoppler_plan, gpu_band_dedoppler

const libbldp = get(ENV, "BLDP_LIB", joinpath(@__DIR__, "..", "libbldp_hip.so"))

# include/bldp.h BLDP_ABI_VERSION this binding is written against
const ABI_VERSION = 5
function __init__()
    v = ccall((:bldp_abi_version, libbldp), Cint, ())
    v == ABI_VERSION || error("libbldp_hip ABI version $v, BLDPHip expects $ABI_VERSION: rebuild it")
end

# bldp_dtype codes (include/bldp.h) and the element type of each code
const GPUElt = Union{Float32,Float64,UInt8,UInt16,UInt32,UInt64,Int8,Int16,Int32,Int64}
const ELTYPES = (Float32, Float64, UInt8, UInt16, UInt32, UInt64, Int8, Int16, Int32, Int64)
dtypecode(::Type{T}) where {T<:GPUElt} = Cint(findfirst(==(T), ELTYPES) - 1)

# fqavfunc values with a GPU implementation (README.md:192-195); anything
# else keeps the reference's host fqav.
opcode(f) = f === sum ? Cint(0) : f === mean ? Cint(1) : f === maximum ? Cint(2) :
            f === minimum ? Cint(3) : nothing
# Statistics' var (corrected), std and median have kernels for Float32 data
# (BLDP_OP_VAR / _STD / _MEDIAN, no time integration); arrays of any other
# element type return nothing here, so the reference's host fqav runs.
# `mad` is this module's (below): BLDP_OP_MAD = 8, code 7 is unassigned.
opcode(f, A) = opcode(f) !== nothing ? opcode(f) : !(A isa Array{Float32,3}) ? nothing :
               f === var ? Cint(4) : f === std ? Cint(5) : f === median ? Cint(6) :
               f === mad ? Cint(8) : nothing

# isless order of a float as unsigned order, and the median by the kernels'
# rule: the middle element of an odd slice, a/2 + b/2 in the element type of
# an even one, NaN when the slice holds a NaN.
_madkey(x::T) where {T<:AbstractFloat} = (u = reinterpret(Unsigned, x); signbit(x) ? ~u : u | ~(typemax(u) >> 1))
function _madmedian(v::AbstractVector{T}) where {T<:AbstractFloat}
    any(isnan, v) && return T(NaN)
    s = sort(v; by=_madkey)
    n = length(s)
    isodd(n) ? s[(n + 1) ÷ 2] : s[n ÷ 2] / 2 + s[n ÷ 2 + 1] / 2
end
function _mad(v::AbstractVector{T}) where {T<:AbstractFloat}
    length(v) <= 1 && return isempty(v) ? T(NaN) : v[1]
    c = _madmedian(v)
    T(Float64(_madmedian(abs.(v .- c))) * 1.4826022185056018)
end
_mad(v::AbstractVector) = _mad(Float64.(v))

"""
    mad(X; dims)

The normalised median absolute deviation of every slice of `X` along `dims`
(StatsBase's `mad(x; normalize=true)`, which has no `dims`, written out over
slices so that it works as a `fqavfunc` / `tavfunc` on the reference's generic
host path): `c = median(x)`, `m = median(abs.(x .- c))`, result
`T(Float64(m) * 1.4826022185056018)` for Float32 / Float64 data and the Float64
product for anything else.  A slice holding a NaN, or more than half one
infinity, gives NaN.  Float32 arrays take the GPU kernels (BLDP_OP_MAD)."""
mad(X::AbstractArray; dims=:) = dims === Colon() ? _mad(vec(X)) : mapslices(_mad, X; dims=dims)

function lasterror()
    buf = Vector{UInt8}(undef, 1024)
    ccall((:bldp_last_error, libbldp), Cint, (Ptr{UInt8}, Csize_t), buf, length(buf))
    unsafe_string(pointer(buf))
end

function check(rc::Integer)
    rc == 0 && return nothing
    msg = lasterror()
    rc == -2 && throw(DimensionMismatch(msg))   # fqavby/tavby does not divide
    rc == -6 && throw(BoundsError(msg))         # window outside the array
    rc == -1 && throw(ArgumentError(msg))
    rc == -8 && throw(SystemError(msg))         # a file read failed or ended early
    error("libbldp_hip error $rc: $msg")
end

"""
    gpu_init(devs=nothing)

bldp_init: validate the GPUs (gfx950), create their worker streams and warm
host-staging pipelines, enable xGMI peer access between them.  Called once per
worker process after `GBT.setupworkers` (src/gbt.jl:12-46) has started it;
optional, since every entry point initialises what it needs on first use.
`nothing` selects every visible device."""
function gpu_init(devs::Union{Nothing,AbstractVector{<:Integer}}=nothing)
    if devs === nothing
        check(ccall((:bldp_init, libbldp), Cint, (Cint, Ptr{Cint}), 0, C_NULL))
    else
        d = Cint.(collect(devs))
        GC.@preserve d check(ccall((:bldp_init, libbldp), Cint, (Cint, Ptr{Cint}), length(d), d))
    end
    nothing
end

"bldp_finalize: drain the devices and free every library-owned resource."
gpu_finalize() = (check(ccall((:bldp_finalize, libbldp), Cint, ())); nothing)

"""
    gpu_pin(A::Array) / gpu_unpin(A::Array)

Page-lock a long-lived host array (bldp_host_register) so gpu_reduce and
gpu_kurtosis copy it at full PCIe rate; the caller keeps `A` alive meanwhile."""
gpu_pin(A::Array) = (check(ccall((:bldp_host_register, libbldp), Cint, (Ptr{Cvoid}, Csize_t),
                                 A, sizeof(A))); A)
gpu_unpin(A::Array) = (check(ccall((:bldp_host_unregister, libbldp), Cint, (Ptr{Cvoid},), A));
                       A)

# Julia index -> (0-based start, count, step) on an axis of length n
axiswin(::Colon, n) = (0, n, 1)
axiswin(i::Integer, n) = (i - 1, 1, 1)                      # sanitizeidxs: i -> i:i
axiswin(r::AbstractRange{<:Integer}, n) = (first(r) - 1, length(r), step(r))

function window(idxs::Tuple, sz)
    @assert length(idxs) == 3 "idxs must have exactly three indices"
    all(i -> i isa Colon, idxs) && return Ptr{Int64}(C_NULL)
    Int64[x for ax in 1:3 for x in axiswin(idxs[ax], sz[ax])]
end

"""
    gpu_reduce(A::Array{Float32,3}, fqavby, tavby=1; f=sum, idxs=(:,:,:), dev=0)

`fqav(A[idxs...], fqavby; f)` fused with the same reduction over `tavby`
spectra, computed on GPU `dev` (bldp_reduce_host_f32)."""
function gpu_reduce(A::Array{Float32,3}, fqavby::Integer, tavby::Integer=1;
                    f=sum, idxs::Tuple=(:, :, :), dev::Integer=0)
    op = opcode(f, A)
    op === nothing && throw(ArgumentError("no GPU kernel for $f"))
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, shp))
    out = Array{Float32,3}(undef, shp...)
    GC.@preserve A win out check(ccall((:bldp_reduce_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{Float32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, op, out))
    out
end

"""
    gpu_reduce(A::Array{T,3}, fqavby, tavby=1; f=sum, idxs=(:,:,:), dev=0) for T other than Float32

The same for integer and Float64 data (SIGPROC nbits 8 / 16 mmaps to UInt8 /
UInt16, src/gbtworkerfunctions.jl:173), with fqav's Julia result type:
bldp_reduce_out_dtype (sum widened to (U)Int64 exactly, mean Float64,
maximum / minimum the input type), reduced on GPU `dev` (bldp_reduce_host)."""
function gpu_reduce(A::Array{T,3}, fqavby::Integer, tavby::Integer=1;
                    f=sum, idxs::Tuple=(:, :, :), dev::Integer=0) where {T<:GPUElt}
    op = opcode(f)
    op === nothing && throw(ArgumentError("no GPU kernel for $f"))
    od = ccall((:bldp_reduce_out_dtype, libbldp), Cint, (Cint, Cint), dtypecode(T), op)
    od < 0 && check(od)
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, shp))
    out = Array{ELTYPES[od + 1],3}(undef, shp...)
    GC.@preserve A win out check(ccall((:bldp_reduce_host, libbldp), Cint,
        (Cint, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{Cvoid}),
        dev, dtypecode(T), A, size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, op, out))
    out
end

"""
    gpu_fqav(A, n; f=sum, tavby=1)

Drop-in for `fqav(A, n; f)` (src/gbtworkerfunctions.jl:16-20): same
pass-through for `n <= 1`, same DimensionMismatch, GPU for sum/mean/maximum/
minimum (and, for Float32 arrays with `tavby <= 1`, var/std/median/mad), the
reference's host code for any other `f` (`mad` of other element types too:
its `dims` method is what that code calls)."""
function gpu_fqav(A, n::Integer; f=sum, tavby::Integer=1, dev::Integer=0)
    (n <= 1 && tavby <= 1) && return A
    if A isa Array{<:GPUElt,3} && opcode(f, A) !== nothing
        return gpu_reduce(A, n, tavby; f, dev)
    end
    tavby <= 1 || throw(ArgumentError("tavby needs a 3-D array and sum/mean/max/min"))
    sz = (n, :, size(A)[2:end]...)
    dropdims(f(reshape(A, sz), dims=1), dims=1)
end

"""
    gpu_kurtosis(A::Array{Float32,3}; idxs=(:,:,:), dev=0, tblock=nothing)

getkurtosis' per-(channel, IF) excess kurtosis over time
(src/gbtworkerfunctions.jl:197-202), computed on GPU `dev`
(bldp_kurtosis_host_f32: window staged on the device, StatsBase recipe,
Float64 result): a `Matrix{Float64}`.  With `tblock = M` the selected spectra
are cut into blocks of M and the result is the `Array{Float64,3}` (nc, ni,
nt / M) of every block's kurtosis (bldp_kurtosis_blocks_host_f32, one call);
M must divide the selected spectra (DimensionMismatch)."""
function gpu_kurtosis(A::Array{Float32,3}; idxs::Tuple=(:, :, :), dev::Integer=0,
                      tblock::Union{Nothing,Integer}=nothing)
    win = window(idxs, size(A))
    if tblock !== nothing
        shp = zeros(Int64, 3)
        GC.@preserve win check(ccall((:bldp_kurtosis_blocks_shape, libbldp), Cint,
            (Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}),
            size(A, 1), size(A, 2), size(A, 3), win, tblock, shp))
        out = Array{Float64,3}(undef, shp...)
        GC.@preserve A win out check(ccall((:bldp_kurtosis_blocks_host_f32, libbldp), Cint,
            (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
            dev, A, size(A, 1), size(A, 2), size(A, 3), win, tblock, out))
        return out
    end
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, 1, 1, shp))
    out = Matrix{Float64}(undef, shp[1], shp[2])
    GC.@preserve A win out check(ccall((:bldp_kurtosis_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, out))
    out
end

"""
    gpu_skewness(A::Array{Float32,3}; idxs=(:,:,:), dev=0, tblock=0)

`map(skewness, eachrow(reshape(data, :, size(data, 3))))` in place of
getkurtosis' line (src/gbtworkerfunctions.jl:200): StatsBase.skewness of every
(channel, IF) row over time with Base.sum's Float32 mean, on GPU `dev`
(bldp_skewness_host_f32).  `tblock = 0`: the whole window, a `Matrix{Float64}`;
`tblock = M`: the `Array{Float64,3}` (nc, ni, nt / M) of every block of M
selected spectra (M must divide them: DimensionMismatch).  Float32 only."""
function gpu_skewness(A::Array{Float32,3}; idxs::Tuple=(:, :, :), dev::Integer=0,
                      tblock::Integer=0)
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    if tblock > 0
        GC.@preserve win check(ccall((:bldp_kurtosis_blocks_shape, libbldp), Cint,
            (Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}),
            size(A, 1), size(A, 2), size(A, 3), win, tblock, shp))
    else
        GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
            (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
            size(A, 1), size(A, 2), size(A, 3), win, 1, 1, shp))
    end
    out = tblock > 0 ? Array{Float64,3}(undef, shp...) : Matrix{Float64}(undef, shp[1], shp[2])
    GC.@preserve A win out check(ccall((:bldp_skewness_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, tblock, out))
    out
end

"""
    gpu_moments(A::Array{Float32,3}; idxs=(:,:,:), dev=0, tblock=0)

Mean, variance, skewness and kurtosis of every (channel, IF) row over time from
one staging of the window on GPU `dev` (bldp_moments_host_f32): a NamedTuple
`(mean, var, skewness, kurtosis)`.  `skewness` and `kurtosis` are what
`gpu_skewness` and `gpu_kurtosis` return, `mean` is `Float64(mean(v))` of the
Float32 row, and `var` is `cm2 / n`, the UNCORRECTED variance both StatsBase
recipes divide by (`var(v; corrected=false)` in their arithmetic, not `var(v)`).
`tblock = 0`: the whole window, four `Matrix{Float64}`; `tblock = M`: four
`Array{Float64,3}` (nc, ni, nt / M), one value per block of M selected spectra
(M must divide them: DimensionMismatch).  Float32 only."""
function gpu_moments(A::Array{Float32,3}; idxs::Tuple=(:, :, :), dev::Integer=0,
                     tblock::Integer=0)
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    if tblock > 0
        GC.@preserve win check(ccall((:bldp_kurtosis_blocks_shape, libbldp), Cint,
            (Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}),
            size(A, 1), size(A, 2), size(A, 3), win, tblock, shp))
    else
        GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
            (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
            size(A, 1), size(A, 2), size(A, 3), win, 1, 1, shp))
    end
    plane() = tblock > 0 ? Array{Float64,3}(undef, shp...) : Matrix{Float64}(undef, shp[1], shp[2])
    m, v, s, k = plane(), plane(), plane(), plane()
    GC.@preserve A win m v s k check(ccall((:bldp_moments_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, tblock, m, v, s, k))
    (mean=m, var=v, skewness=s, kurtosis=k)
end

"""
    gpu_kurtosis(A::Array{T,3}; idxs=(:,:,:), dev=0, tblock=nothing) for T other than Float32

StatsBase.kurtosis of integer or Float64 rows (Float64 throughout: Base.sum's
pairwise mean, sequential moments), on GPU `dev` (bldp_kurtosis_host).  With
`tblock = M`: one such call per block of M selected spectra, stacked along the
third axis."""
function gpu_kurtosis(A::Array{T,3}; idxs::Tuple=(:, :, :), dev::Integer=0,
                      tblock::Union{Nothing,Integer}=nothing) where {T<:GPUElt}
    win = window(idxs, size(A))
    if tblock !== nothing
        shp = zeros(Int64, 3)
        GC.@preserve win check(ccall((:bldp_kurtosis_blocks_shape, libbldp), Cint,
            (Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}),
            size(A, 1), size(A, 2), size(A, 3), win, tblock, shp))
        out = Array{Float64,3}(undef, shp...)
        # (window(...) of (:,:,:) is a null pointer: spell the whole array out)
        bwin = win isa Ptr ? Int64[0, size(A, 1), 1, 0, size(A, 2), 1, 0, size(A, 3), 1] : copy(win)
        t0 = bwin[7]
        bwin[8] = tblock
        for b in 1:shp[3]
            bwin[7] = t0 + (b - 1) * tblock * bwin[9]
            o = view(out, :, :, b)
            GC.@preserve A bwin out check(ccall((:bldp_kurtosis_host, libbldp), Cint,
                (Cint, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                dev, dtypecode(T), A, size(A, 1), size(A, 2), size(A, 3), bwin, pointer(o)))
        end
        return out
    end
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, 1, 1, shp))
    out = Matrix{Float64}(undef, shp[1], shp[2])
    GC.@preserve A win out check(ccall((:bldp_kurtosis_host, libbldp), Cint,
        (Cint, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
        dev, dtypecode(T), A, size(A, 1), size(A, 2), size(A, 3), win, out))
    out
end

# tavfunc values with a time-axis kernel of their own (csrc/tstats.hip)
statcode(f) = f === var ? Cint(4) : f === std ? Cint(5) : f === median ? Cint(6) :
              f === mad ? Cint(8) : nothing

"""
    gpu_tstat(A::Array{Float32,3}, tavby; f=median, idxs=(:,:,:), dev=0) -> Array{Float32,3}

`f` (Statistics' `var`, `std` or `median`, or this module's `mad`) of every block of `tavby` selected
spectra of every (channel, IF) column, fqav's rule on axis 3:
`R[c, i, b] = f(A[idxs...][c, i, (b-1)*tavby+1 : b*tavby])`, computed on GPU `dev`
(bldp_tstat_host_f32: the window staged on the device).  `tavby` must divide
the selected spectra (DimensionMismatch); `tavby <= 1` returns the window."""
function gpu_tstat(A::Array{Float32,3}, tavby::Integer; f=median, idxs::Tuple=(:, :, :),
                   dev::Integer=0)
    op = statcode(f)
    op === nothing && throw(ArgumentError("gpu_tstat takes var, std, median or mad, not $f"))
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_tstat_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, tavby, shp))
    out = Array{Float32,3}(undef, shp...)
    GC.@preserve A win out check(ccall((:bldp_tstat_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Cint, Ptr{Float32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, tavby, op, out))
    out
end

"""
    gpu_tstat(in::Ptr{Float32}, dims, tavby, out::Ptr{Float32}; f=median, win=C_NULL,
              out_ld=nothing, stream=C_NULL)

The same on DEVICE memory (bldp_tstat_f32; asynchronous on `stream`): `in` a
(nchan, nif, ntime) = `dims` device array, `win` the 9-element window or
C_NULL, element (c, i, b) written at `out[c + i*out_ld[1] + b*out_ld[2]]`
(0-based; dense by default), e.g. a bank's slot of a stitched product."""
function gpu_tstat(in::Ptr{Float32}, dims::NTuple{3,Integer}, tavby::Integer, out::Ptr{Float32};
                   f=median, win=Ptr{Int64}(C_NULL), out_ld=nothing, stream::Ptr{Cvoid}=C_NULL)
    op = statcode(f)
    op === nothing && throw(ArgumentError("gpu_tstat takes var, std, median or mad, not $f"))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_tstat_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, tavby, shp))
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2]) : out_ld
    GC.@preserve win check(ccall((:bldp_tstat_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Cint, Ptr{Float32}, Int64, Int64,
         Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, tavby, op, out, ld[1], ld[2], stream))
    (shp[1], shp[2], shp[3])
end

# ---- quantile(p): bldp_quantile_* (no op code: the entry points carry p) -------
_checkp(p) = (0 <= p <= 1) || throw(ArgumentError("quantile: p=$p is outside [0, 1]"))

# Statistics.quantile's default (type 7) by the kernels' rule (include/bldp.h):
# isless order, the index and weight in Float64, a + g * (b - a) with the
# difference rounded in the element type where both are finite, else
# (1 - g) * a + g * b; NaN when the slice holds a NaN (Statistics throws there).
function _quantile(v::AbstractVector{T}, p::Real) where {T<:AbstractFloat}
    n = length(v)
    n <= 1 && return isempty(v) ? T(NaN) : v[1]
    any(isnan, v) && return T(NaN)
    s = sort(v; by=_madkey)
    pp = Float64(p)
    m = 1.0 + pp * (1.0 - 1.0 - 1.0)
    aleph = n * pp + m
    j = clamp(trunc(Int, aleph), 1, n - 1)
    g = clamp(aleph - j, 0.0, 1.0)
    a, b = s[j], s[j + 1]
    r = isfinite(a) && isfinite(b) ? Float64(a) + g * Float64(b - a) :
        (1.0 - g) * Float64(a) + g * Float64(b)
    T(r)
end
_quantile(v::AbstractVector, p::Real) = _quantile(Float64.(v), p)

"""
    quantile(X, p; dims)

`Statistics.quantile(slice, p)` (the default definition, type 7) of every slice
of `X` along `dims`, which Statistics' own method does not take; this module's
function, in the style of `mad(X; dims)` (qualify it as `BLDPHip.quantile` next
to `using Statistics`).  A Float32 (nchan, nif, ntime) array with `dims = 1` or
`dims = 3` runs on the GPU (bldp_quantile_host_f32, one block of `size(X, dims)`
per slice); anything else takes the same rule on the host.  A slice holding a
NaN gives NaN.  `quantile(X, 0.5; dims)` of an even slice is `a + 0.5 (b - a)`,
which may differ from `median`'s `a/2 + b/2` in the last bit."""
function quantile(X::AbstractArray, p::Real; dims=:, dev::Integer=0)
    _checkp(p)
    dims === Colon() && return _quantile(vec(X), p)
    if X isa Array{Float32,3} && (dims == 1 || dims == 3) && size(X, dims) > 1
        return gpu_quantile(X, size(X, dims), p; axis=dims - 1, dev)
    end
    mapslices(v -> _quantile(v, p), X; dims=dims)
end

"""
    gpu_quantile(A::Array{Float32,3}, n, p; axis=0, idxs=(:,:,:), dev=0) -> Array{Float32,3}

quantile(p) of every block of `n` selected channels (`axis = 0`, an fqavfunc) or
`n` selected spectra (`axis = 2`, a tavfunc) of the window, computed on GPU
`dev` (bldp_quantile_host_f32: the window staged on the device).  `n` must
divide the axis (DimensionMismatch); `n <= 1` returns the window."""
function gpu_quantile(A::Array{Float32,3}, n::Integer, p::Real; axis::Integer=0,
                      idxs::Tuple=(:, :, :), dev::Integer=0)
    _checkp(p)
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_quantile_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, axis, n, shp))
    out = Array{Float32,3}(undef, shp...)
    GC.@preserve A win out check(ccall((:bldp_quantile_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64, Ptr{Float32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, axis, n, p, out))
    out
end

"""
    gpu_quantile(in::Ptr{Float32}, dims, n, p, out::Ptr{Float32}; axis=0, win=C_NULL,
                 out_ld=nothing, stream=C_NULL)

The same on DEVICE memory (bldp_quantile_f32; asynchronous on `stream`): output
element (c, i, t) written at `out[c + i*out_ld[1] + t*out_ld[2]]` (0-based;
dense by default).  Returns the output's dims."""
function gpu_quantile(in::Ptr{Float32}, dims::NTuple{3,Integer}, n::Integer, p::Real,
                      out::Ptr{Float32}; axis::Integer=0, win=Ptr{Int64}(C_NULL), out_ld=nothing,
                      stream::Ptr{Cvoid}=C_NULL)
    _checkp(p)
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_quantile_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, axis, n, shp))
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2]) : out_ld
    GC.@preserve win check(ccall((:bldp_quantile_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64, Ptr{Float32}, Int64,
         Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, axis, n, p, out, ld[1], ld[2], stream))
    (shp[1], shp[2], shp[3])
end

"""
    gpu_quantile_plan(dims, n, p; axis=0, win=C_NULL) -> Vector{Int64}

The launch plan of that call (bldp_quantile_plan_f32; needs no GPU): the
median's plan of the axis and shape, the 0-based lower rank in its
workspace-bytes slot (the 7th entry on axis 0, the 6th on axis 2)."""
function gpu_quantile_plan(dims::NTuple{3,Integer}, n::Integer, p::Real; axis::Integer=0,
                           win=Ptr{Int64}(C_NULL))
    _checkp(p)
    info = zeros(Int64, 8)
    GC.@preserve win check(ccall((:bldp_quantile_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64, Ptr{Float32},
         Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, axis, n, p, C_NULL, info))
    info
end

"""
    gpu_band_quantile(banks::Vector{Ptr{Float32}}, dims, n, p, out::Ptr{Float32}; axis=0,
                      win=C_NULL, stream=C_NULL)

quantile(p) of every bank of a band resident on one GPU, stitched in bank order
in one launch (bldp_band_quantile_f32); `out` is the dense vcat of the banks."""
function gpu_band_quantile(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer}, n::Integer,
                           p::Real, out::Ptr{Float32}; axis::Integer=0, win=Ptr{Int64}(C_NULL),
                           stream::Ptr{Cvoid}=C_NULL)
    _checkp(p)
    GC.@preserve banks win check(ccall((:bldp_band_quantile_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64,
         Ptr{Float32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, axis, n, p, out, stream))
    nothing
end

# ---- quantiles(ps): bldp_quantiles_* (several quantiles from one selection) -----
const MAX_QUANTILES = 8  # BLDP_MAX_QUANTILES: probabilities one launch takes

function _checkps(ps)
    isempty(ps) && throw(ArgumentError("quantiles: ps is empty"))
    foreach(_checkp, ps)
    collect(Float64, ps)
end

"""
    gpu_quantiles(A::Array{Float32,3}, n, ps; axis=0, idxs=(:,:,:), dev=0) -> Array{Float32,4}

`quantile(block, ps)` (Julia's vector form) of every block of `n` selected
channels (`axis = 0`) or `n` selected spectra (`axis = 2`) of the window, on
GPU `dev` (bldp_quantiles_host_f32): every block is read and its ranks selected
once.  The result has `length(ps)` planes on a new last axis; plane `k` is bit
for bit `gpu_quantile(A, n, ps[k]; axis, idxs, dev)`.  `ps` may be unsorted and
may repeat; more than $(MAX_QUANTILES) go in several calls into the one array."""
function gpu_quantiles(A::Array{Float32,3}, n::Integer, ps; axis::Integer=0,
                       idxs::Tuple=(:, :, :), dev::Integer=0)
    pv = _checkps(ps)
    win = window(idxs, size(A))
    shp = zeros(Int64, 4)
    GC.@preserve win check(ccall((:bldp_quantiles_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, axis, n, 1, shp))
    out = Array{Float32,4}(undef, shp[1], shp[2], shp[3], length(pv))
    plane = shp[1] * shp[2] * shp[3]
    for k0 in 1:MAX_QUANTILES:length(pv)
        part = pv[k0:min(k0 + MAX_QUANTILES - 1, length(pv))]
        GC.@preserve A win out part check(ccall((:bldp_quantiles_host_f32, libbldp), Cint,
            (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint,
             Ptr{Float64}, Ptr{Float32}),
            dev, A, size(A, 1), size(A, 2), size(A, 3), win, axis, n, length(part), part,
            pointer(out, (k0 - 1) * plane + 1)))
    end
    out
end

"""
    gpu_quantiles(in::Ptr{Float32}, dims, n, ps, out::Ptr{Float32}; axis=0, win=C_NULL,
                  out_ld=nothing, stream=C_NULL)

The same on DEVICE memory for at most $(MAX_QUANTILES) probabilities
(bldp_quantiles_f32; asynchronous on `stream`): element (c, i, t) of plane k at
`out[c + i*out_ld[1] + t*out_ld[2] + k*out_ld[3]]` (0-based; dense by default).
Returns the output's dims."""
function gpu_quantiles(in::Ptr{Float32}, dims::NTuple{3,Integer}, n::Integer, ps,
                       out::Ptr{Float32}; axis::Integer=0, win=Ptr{Int64}(C_NULL), out_ld=nothing,
                       stream::Ptr{Cvoid}=C_NULL)
    pv = _checkps(ps)
    shp = zeros(Int64, 4)
    GC.@preserve win check(ccall((:bldp_quantiles_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, axis, n, length(pv), shp))
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2], shp[1] * shp[2] * shp[3]) : out_ld
    GC.@preserve win pv check(ccall((:bldp_quantiles_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint, Ptr{Float64},
         Ptr{Float32}, Int64, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, axis, n, length(pv), pv, out, ld[1], ld[2], ld[3],
        stream))
    (shp[1], shp[2], shp[3], shp[4])
end

"""
    gpu_quantiles_plan(dims, n, ps; axis=0, win=C_NULL) -> Vector{Int64}

The launch plan of that call (bldp_quantiles_plan_f32; needs no GPU): the
median's plan of the axis and shape in the first eight entries, then the count
of distinct ranks selected and the count of reads of the block."""
function gpu_quantiles_plan(dims::NTuple{3,Integer}, n::Integer, ps; axis::Integer=0,
                            win=Ptr{Int64}(C_NULL))
    pv = _checkps(ps)
    info = zeros(Int64, 10)
    GC.@preserve win pv check(ccall((:bldp_quantiles_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint, Ptr{Float64},
         Ptr{Float32}, Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, axis, n, length(pv), pv, C_NULL, info))
    info
end

"""
    gpu_band_quantiles(banks::Vector{Ptr{Float32}}, dims, n, ps, out::Ptr{Float32}; axis=0,
                       win=C_NULL, stream=C_NULL)

quantiles(ps), at most $(MAX_QUANTILES), of every bank of a band resident on one
GPU, stitched in bank order in one launch (bldp_band_quantiles_f32); `out` holds
the dense planes of the vcat of the banks one after the other."""
function gpu_band_quantiles(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer}, n::Integer,
                            ps, out::Ptr{Float32}; axis::Integer=0, win=Ptr{Int64}(C_NULL),
                            stream::Ptr{Cvoid}=C_NULL)
    pv = _checkps(ps)
    GC.@preserve banks win pv check(ccall((:bldp_band_quantiles_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint,
         Ptr{Float64}, Ptr{Float32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, axis, n, length(pv), pv, out,
        stream))
    nothing
end

# ---- outliers: bldp_outliers_* (median, mad, count and flags from one launch) ----
function _checknsigma(nsigma)
    (nsigma >= 0 && isfinite(nsigma)) ||
        throw(ArgumentError("outliers: nsigma=$nsigma is not a finite number >= 0"))
    Float64(nsigma)
end

function _outliers_shape(dims, win, axis, n)
    shp = zeros(Int64, 3)
    mshp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_outliers_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Ptr{Int64}, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, axis, n, shp, mshp))
    shp, mshp
end

"""
    gpu_outliers(A::Array{Float32,3}, n; axis=2, nsigma=5.0, idxs=(:,:,:), mask=false, dev=0)
        -> (median, mad, count[, mask])

The median, the scaled mad (`mad(block; normalize=true)`), the count of outliers
and, with `mask=true`, the outlier flags of every block of `n` selected channels
(`axis = 0`) or `n` selected spectra (`axis = 2`) of the window, on GPU `dev`
(bldp_outliers_host_f32): a sample is flagged when `abs(x - median) >
Float32(nsigma * mad)`, strictly, and a block whose median or mad is NaN flags
nothing.  `median` and `mad` are `Float32`, `count` is `UInt32`, each sized as
`gpu_quantile`'s result; `mask` is the window's `UInt8` array."""
function gpu_outliers(A::Array{Float32,3}, n::Integer; axis::Integer=2, nsigma::Real=5.0,
                      idxs::Tuple=(:, :, :), mask::Bool=false, dev::Integer=0)
    ns = _checknsigma(nsigma)
    win = window(idxs, size(A))
    shp, mshp = _outliers_shape(size(A), win, axis, n)
    med = Array{Float32,3}(undef, shp[1], shp[2], shp[3])
    sc = Array{Float32,3}(undef, shp[1], shp[2], shp[3])
    cnt = Array{UInt32,3}(undef, shp[1], shp[2], shp[3])
    msk = mask ? Array{UInt8,3}(undef, mshp[1], mshp[2], mshp[3]) : nothing
    GC.@preserve A win med sc cnt msk check(ccall((:bldp_outliers_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64, Ptr{Float32},
         Ptr{Float32}, Ptr{UInt32}, Ptr{UInt8}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, axis, n, ns, med, sc, cnt,
        mask ? pointer(msk) : Ptr{UInt8}(C_NULL)))
    mask ? (med, sc, cnt, msk) : (med, sc, cnt)
end

"""
    gpu_outliers(in::Ptr{Float32}, dims, n, med, mad, count, mask; axis=2, nsigma=5.0,
                 win=C_NULL, out_ld=nothing, stream=C_NULL)

The same on DEVICE memory (bldp_outliers_f32; asynchronous on `stream`, one
launch): element (c, i, t) of `med`, `mad` and `count` at `[c + i*out_ld[1] +
t*out_ld[2]]` (0-based; dense by default), `mask` the dense window.  Any of the
four pointers may be `C_NULL`: that output is neither formed nor stored.
Returns the dims of the planes and of the mask."""
function gpu_outliers(in::Ptr{Float32}, dims::NTuple{3,Integer}, n::Integer, med::Ptr{Float32},
                      mad::Ptr{Float32}, count::Ptr{UInt32}, mask::Ptr{UInt8};
                      axis::Integer=2, nsigma::Real=5.0, win=Ptr{Int64}(C_NULL), out_ld=nothing,
                      stream::Ptr{Cvoid}=C_NULL)
    ns = _checknsigma(nsigma)
    shp, mshp = _outliers_shape(dims, win, axis, n)
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2]) : out_ld
    GC.@preserve win check(ccall((:bldp_outliers_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64, Ptr{Float32},
         Ptr{Float32}, Ptr{UInt32}, Ptr{UInt8}, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, axis, n, ns, med, mad, count, mask, ld[1], ld[2],
        stream))
    (shp[1], shp[2], shp[3]), (mshp[1], mshp[2], mshp[3])
end

"""
    gpu_outliers_plan(dims, n; axis=2, win=C_NULL, mask=false) -> Vector{Int64}

The launch plan of that call (bldp_outliers_plan_f32; needs no GPU): mad's plan
of the axis and shape in the first eight entries, then the count of reads of the
block and whether a mask is written."""
function gpu_outliers_plan(dims::NTuple{3,Integer}, n::Integer; axis::Integer=2,
                           win=Ptr{Int64}(C_NULL), mask::Bool=false)
    info = zeros(Int64, 10)
    GC.@preserve win check(ccall((:bldp_outliers_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Cint, Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, axis, n, mask ? 1 : 0, info))
    info
end

"""
    gpu_band_outliers(banks::Vector{Ptr{Float32}}, dims, n, med, mad, count, mask; axis=2,
                      nsigma=5.0, win=C_NULL, stream=C_NULL)

outliers of every bank of a band resident on one GPU, stitched in bank order in
one launch (bldp_band_outliers_f32): `med`, `mad` and `count` hold the dense
vcat of the banks' planes, `mask` the vcat of their windows."""
function gpu_band_outliers(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer}, n::Integer,
                           med::Ptr{Float32}, mad::Ptr{Float32}, count::Ptr{UInt32},
                           mask::Ptr{UInt8}; axis::Integer=2, nsigma::Real=5.0,
                           win=Ptr{Int64}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    ns = _checknsigma(nsigma)
    GC.@preserve banks win check(ccall((:bldp_band_outliers_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Cint, Int64, Float64,
         Ptr{Float32}, Ptr{Float32}, Ptr{UInt32}, Ptr{UInt8}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, axis, n, ns, med, mad, count, mask,
        stream))
    nothing
end

# ---- masked reduce: bldp_*masked_reduce_* (a window over its unflagged samples) ----
_maskedop(f) = f === sum ? Cint(0) : f === mean ? Cint(1) :
               throw(ArgumentError("masked reduce takes sum or mean, not $f"))
# mask_ld of a UInt8 array over a window of size wsz: an axis of length 1 is a
# broadcast (stride 0)
function _mask_ld(msk::Array{UInt8,3}, wsz)
    all(size(msk, a) == 1 || size(msk, a) == wsz[a] for a in 1:3) ||
        throw(DimensionMismatch("mask $(size(msk)) does not broadcast to the window $wsz"))
    Int64[size(msk, a) == 1 ? 0 : stride(msk, a) for a in 1:3]
end

"""
    gpu_masked_reduce(A::Array{Float32,3}, msk::Array{UInt8,3}, fqavby=1, tavby=1; f=sum,
                      idxs=(:,:,:), dev=0) -> (data, kept)

`f` (`sum` or `mean`) of the samples of every `fqavby` x `tavby` block of
`A[idxs...]` whose byte of `msk` is 0, and how many there were, on GPU `dev`
(bldp_masked_reduce_host_f32).  `msk` has the window's size, any axis of which
may be 1 (a broadcast: a bad-channel list is `(nc, 1, 1)`); `gpu_outliers`' mask
goes in as it is.  A flagged `NaN` or `Inf` leaves the result finite; a block
with nothing kept gives `0.0f0` (`sum`) or `NaN32` (`mean`).  `data` is `Float32`,
`kept` `Int32`: the weight of each product."""
function gpu_masked_reduce(A::Array{Float32,3}, msk::Array{UInt8,3}, fqavby::Integer=1,
                           tavby::Integer=1; f=sum, idxs::Tuple=(:, :, :), dev::Integer=0)
    op = _maskedop(f)
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, shp))
    ld = _mask_ld(msk, (shp[1] * max(fqavby, 1), shp[2], shp[3] * max(tavby, 1)))
    data = Array{Float32,3}(undef, shp...)
    kept = Array{UInt32,3}(undef, shp...)
    GC.@preserve A msk win ld data kept check(ccall((:bldp_masked_reduce_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{UInt8},
         Ptr{Int64}, Ptr{Float32}, Ptr{UInt32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, op, msk, ld, data, kept))
    data, Int32.(kept)   # counts are < 2^31
end

"""
    gpu_masked_reduce(in::Ptr{Float32}, dims, mask::Ptr{UInt8}, out, kept, fqavby=1, tavby=1;
                      f=sum, win=C_NULL, mask_ld=C_NULL, out_ld=nothing, stream=C_NULL)

The same on DEVICE memory (bldp_masked_reduce_f32; asynchronous on `stream`, one
launch): flag (c, i, t) of the window at `mask[c*mask_ld[1] + i*mask_ld[2] +
t*mask_ld[3]]` (0-based c, i, t; `C_NULL`: dense), element (c, i, t) of `out` and
`kept` at `[c + i*out_ld[1] + t*out_ld[2]]` (dense by default).  `out` or `kept`
may be `C_NULL`, not both.  Returns the dims of the outputs."""
function gpu_masked_reduce(in::Ptr{Float32}, dims::NTuple{3,Integer}, mask::Ptr{UInt8},
                           out::Ptr{Float32}, kept::Ptr{UInt32}, fqavby::Integer=1,
                           tavby::Integer=1; f=sum, win=Ptr{Int64}(C_NULL),
                           mask_ld=Ptr{Int64}(C_NULL), out_ld=nothing, stream::Ptr{Cvoid}=C_NULL)
    op = _maskedop(f)
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, fqavby, tavby, shp))
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2]) : out_ld
    GC.@preserve win mask_ld check(ccall((:bldp_masked_reduce_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{UInt8},
         Ptr{Int64}, Ptr{Float32}, Ptr{UInt32}, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, fqavby, tavby, op, mask, mask_ld, out, kept, ld[1],
        ld[2], stream))
    (shp[1], shp[2], shp[3])
end

"""
    gpu_band_masked_reduce(banks::Vector{Ptr{Float32}}, dims, mask, out, kept, fqavby=1,
                           tavby=1; f=sum, win=C_NULL, mask_ld=C_NULL, stream=C_NULL)

The masked reduce of every bank of a band resident on one GPU in one launch
(bldp_band_masked_reduce_f32): `out` and `kept` hold the dense vcat of the banks'
results; bank b's channel c is channel `b*nc + c` of the mask (`C_NULL` strides:
the dense vcat of the banks' windows, `gpu_band_outliers`' mask)."""
function gpu_band_masked_reduce(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer},
                                mask::Ptr{UInt8}, out::Ptr{Float32}, kept::Ptr{UInt32},
                                fqavby::Integer=1, tavby::Integer=1; f=sum,
                                win=Ptr{Int64}(C_NULL), mask_ld=Ptr{Int64}(C_NULL),
                                stream::Ptr{Cvoid}=C_NULL)
    op = _maskedop(f)
    GC.@preserve banks win mask_ld check(ccall((:bldp_band_masked_reduce_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint,
         Ptr{UInt8}, Ptr{Int64}, Ptr{Float32}, Ptr{UInt32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, fqavby, tavby, op, mask, mask_ld,
        out, kept, stream))
    nothing
end

# ---- histogram: bldp_*histogram_* (sample counts per bin of every block) ----
"""
    gpu_histogram(A::Array{Float32,3}, nbins, lo, hi; fqavby=1, tavby=nothing,
                  idxs=(:,:,:), dev=0) -> (counts, below, above, nan, edges)

The sample counts of every `fqavby` x `tavby` block of `A[idxs...]` (`tavby` or
`fqavby` `nothing`: the whole selected range of that axis) in `nbins` equal bins
of `[lo, hi)`, on GPU `dev` (bldp_histogram_host_f32; the rule of include/bldp.h).
`counts` is `Int32` `(nc/F, ni, nt/T, nbins)`; `below`, `above` and `nan`
`(nc/F, ni, nt/T)` count the samples under `lo`, at or over `hi` and the NaNs.
The counts of a block add up to `F*T` and are exact.  `edges`: the `nbins + 1`
`Float64` bin edges, a reading aid only."""
function gpu_histogram(A::Array{Float32,3}, nbins::Integer, lo::Real, hi::Real; fqavby=1,
                       tavby=nothing, idxs::Tuple=(:, :, :), dev::Integer=0)
    win = window(idxs, size(A))
    nc, nt = win isa Ptr ? (size(A, 1), size(A, 3)) : (win[2], win[8])   # (all colons: no window)
    F = fqavby === nothing ? max(nc, 1) : fqavby
    T = tavby === nothing ? max(nt, 1) : tavby
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, F, T, shp))
    out = Array{UInt32,4}(undef, shp[1], shp[2], shp[3], max(nbins, 0) + 3)
    GC.@preserve A win out check(ccall((:bldp_histogram_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Float64,
         Float64, Ptr{UInt32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, F, T, nbins, lo, hi, out))
    c = Int32.(out)   # counts are < 2^31
    lo32, hi32 = Float64(Float32(lo)), Float64(Float32(hi))
    edges = [lo32 + k * (hi32 - lo32) / nbins for k in 0:nbins]
    (c[:, :, :, 1:nbins], c[:, :, :, nbins + 1], c[:, :, :, nbins + 2], c[:, :, :, nbins + 3],
     edges)
end

"""
    gpu_histogram(in::Ptr{Float32}, dims, nbins, lo, hi, out::Ptr{UInt32}, fqavby=1, tavby=1;
                  win=C_NULL, out_ld=nothing, stream=C_NULL)

The same on DEVICE memory (bldp_histogram_f32; asynchronous on `stream`): plane q
(`0:nbins-1` the bins, `nbins` below, `nbins+1` above, `nbins+2` nan) of block
(c, i, t) at `out[c + i*out_ld[1] + t*out_ld[2] + q*out_ld[3]]` (0-based; dense by
default).  `out` may hold anything beforehand.  Returns the output's dims."""
function gpu_histogram(in::Ptr{Float32}, dims::NTuple{3,Integer}, nbins::Integer, lo::Real,
                       hi::Real, out::Ptr{UInt32}, fqavby::Integer=1, tavby::Integer=1;
                       win=Ptr{Int64}(C_NULL), out_ld=nothing, stream::Ptr{Cvoid}=C_NULL)
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, fqavby, tavby, shp))
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2], shp[1] * shp[2] * shp[3]) : out_ld
    GC.@preserve win check(ccall((:bldp_histogram_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Float64, Float64,
         Ptr{UInt32}, Int64, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, fqavby, tavby, nbins, lo, hi, out, ld[1], ld[2],
        ld[3], stream))
    (shp[1], shp[2], shp[3], nbins + 3)
end

"""
    gpu_histogram_plan(dims, nbins, lo, hi, fqavby=1, tavby=1; win=C_NULL) -> Vector{Int64}

The launch plan of that call (bldp_histogram_plan_f32; launches nothing): {path
(0 block, 1 block_split, 2 lanes, 3 lanes_tsplit), workgroups per bank, chunks per
block, blocks per workgroup, LDS bytes, replicas, workspace bytes, vector loads,
lanes along the channels, rows per chunk}."""
function gpu_histogram_plan(dims::NTuple{3,Integer}, nbins::Integer, lo::Real, hi::Real,
                            fqavby::Integer=1, tavby::Integer=1; win=Ptr{Int64}(C_NULL))
    info = zeros(Int64, 10)
    GC.@preserve win info check(ccall((:bldp_histogram_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Float64, Float64,
         Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, fqavby, tavby, nbins, lo, hi, info))
    info
end

"""
    gpu_band_histogram(banks::Vector{Ptr{Float32}}, dims, nbins, lo, hi, out::Ptr{UInt32},
                       fqavby=1, tavby=1; win=C_NULL, stream=C_NULL)

The histogram of every bank of a band resident on one GPU in one launch
(bldp_band_histogram_f32): `out` holds the dense `(nbank*nco, ni, nto, nbins + 3)`
vcat of the banks' results."""
function gpu_band_histogram(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer},
                            nbins::Integer, lo::Real, hi::Real, out::Ptr{UInt32},
                            fqavby::Integer=1, tavby::Integer=1; win=Ptr{Int64}(C_NULL),
                            stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve banks win check(ccall((:bldp_band_histogram_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Float64,
         Float64, Ptr{UInt32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, fqavby, tavby, nbins, lo, hi, out,
        stream))
    nothing
end

# ---- hits: bldp_*hits_* (the flagged samples of a window as an ordered list) ----
"""
    gpu_hits(A::Array{Float32,3}, msk::Array{UInt8,3}; maxhits=nothing, idxs=(:,:,:), dev=0)
        -> (total, index, value)

`findall(!iszero, msk)` and `A[idxs...][msk]` on GPU `dev` (bldp_hits_host_f32;
the rule of include/bldp.h).  `msk` has the window's size, any axis of which may
be 1 (a broadcast); `gpu_outliers`' mask goes in as it is.  `total` is the number
of flagged samples, always exact; `index` (`Int64`, 1-based linear indices of the
window, ascending: `CartesianIndices(size)[index]` gives channel, IF and time)
and `value` (`Float32`, the samples' bits untouched) hold the first
`min(total, maxhits)` of them (`maxhits=nothing`: all)."""
function gpu_hits(A::Array{Float32,3}, msk::Array{UInt8,3}; maxhits=nothing,
                  idxs::Tuple=(:, :, :), dev::Integer=0)
    maxhits === nothing || maxhits >= 0 || throw(ArgumentError("maxhits=$maxhits is negative"))
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, 1, 1, shp))
    ld = _mask_ld(msk, (shp[1], shp[2], shp[3]))
    total = zeros(UInt64, 1)
    call(cap, idx, val) = GC.@preserve A msk win ld idx val total check(
        ccall((:bldp_hits_host_f32, libbldp), Cint,
              (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int64,
               Ptr{Int64}, Ptr{Float32}, Ptr{UInt64}),
              dev, A, size(A, 1), size(A, 2), size(A, 3), win, msk, ld, cap, idx, val, total))
    cap = maxhits
    if cap === nothing   # count, then list exactly
        call(0, Ptr{Int64}(C_NULL), Ptr{Float32}(C_NULL))
        cap = Int64(total[1])
    end
    idx = Vector{Int64}(undef, cap)
    val = Vector{Float32}(undef, cap)
    call(cap, idx, val)
    n = min(Int64(total[1]), cap)
    Int64(total[1]), idx[1:n] .+ 1, val[1:n]
end

"""
    gpu_hits(in::Ptr{Float32}, dims, mask::Ptr{UInt8}, cap, idx::Ptr{Int64}, val::Ptr{Float32},
             total::Ptr{UInt64}; win=C_NULL, mask_ld=C_NULL, stream=C_NULL)

The same on DEVICE memory (bldp_hits_f32; asynchronous on `stream`, `total` a
device pointer too): flag (c, i, t) of the window at `mask[c*mask_ld[1] +
i*mask_ld[2] + t*mask_ld[3]]` (0-based; `C_NULL`: dense).  Entries
`j < min(total, cap)` of `idx` and `val` are written; either may be `C_NULL`.
The indices in `idx` are 0-BASED as the library writes them: add 1 after the
copy back."""
function gpu_hits(in::Ptr{Float32}, dims::NTuple{3,Integer}, mask::Ptr{UInt8}, cap::Integer,
                  idx::Ptr{Int64}, val::Ptr{Float32}, total::Ptr{UInt64};
                  win=Ptr{Int64}(C_NULL), mask_ld=Ptr{Int64}(C_NULL),
                  stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve win mask_ld check(ccall((:bldp_hits_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int64,
         Ptr{Int64}, Ptr{Float32}, Ptr{UInt64}, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, mask, mask_ld, cap, idx, val, total, stream))
    nothing
end

"""
    gpu_hits_plan(dims, cap=1; win=C_NULL, mask_ld=C_NULL) -> Vector{Int64}

The launch plan of that call (bldp_hits_plan_f32; launches nothing): {mask load
form (0 byte, 1 wide, 2 row-uniform), elements per tile, tiles, workspace bytes,
scan chunks, flags per lane per load, launches, 0, 0, 0}."""
function gpu_hits_plan(dims::NTuple{3,Integer}, cap::Integer=1; win=Ptr{Int64}(C_NULL),
                       mask_ld=Ptr{Int64}(C_NULL))
    info = zeros(Int64, 10)
    GC.@preserve win mask_ld info check(ccall((:bldp_hits_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int64,
         Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, C_NULL, mask_ld, cap, info))
    info
end

"""
    gpu_band_hits(banks::Vector{Ptr{Float32}}, dims, mask, cap, idx, val, total;
                  win=C_NULL, mask_ld=C_NULL, stream=C_NULL)

The list of a band resident on one GPU (bldp_band_hits_f32): the window is the
vcat `(nbank*nc, ni, nt)` of the banks' windows, bank b's channel c is channel
`b*nc + c` of the mask and of the linear index (`C_NULL` strides: the dense vcat,
`gpu_band_outliers`' mask).  0-BASED indices, as the device form."""
function gpu_band_hits(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer}, mask::Ptr{UInt8},
                       cap::Integer, idx::Ptr{Int64}, val::Ptr{Float32}, total::Ptr{UInt64};
                       win=Ptr{Int64}(C_NULL), mask_ld=Ptr{Int64}(C_NULL),
                       stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve banks win mask_ld check(ccall((:bldp_band_hits_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int64,
         Ptr{Int64}, Ptr{Float32}, Ptr{UInt64}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, mask, mask_ld, cap, idx, val, total,
        stream))
    nothing
end

# ---- fold / unfold: bldp_*fold_* and bldp_*unfold_* (a window over its coarse channels) ----
_unfoldop(how) = how === :divide ? Cint(0) : how === :subtract ? Cint(1) :
                 throw(ArgumentError("unfold takes :divide or :subtract, not $how"))
# (nfpc, ni, nto) of a fold; tavby = nothing: the whole selected time range
function _fold_shape(sz, win, nfpc, tavby)
    shp = zeros(Int64, 3)
    T = tavby === nothing ? max(win[8], 1) : tavby
    GC.@preserve win check(ccall((:bldp_fold_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        sz[1], sz[2], sz[3], win, nfpc, T, shp))
    shp, T
end

"""
    gpu_fold(A::Array{Float32,3}, nfpc; tavby=nothing, f=mean, mask=nothing, idxs=(:,:,:),
             dev=0) -> (data, kept)

The profile of `A[idxs...]` over its coarse channels on GPU `dev`
(bldp_fold_host_f32): selected channel c has fine index `c mod nfpc`, and element
`(k, i, t')` of `data` is `f` (`sum` or `mean`) of the samples of fine index k of
every coarse channel and of the `tavby` spectra of time block t' (`nothing`: the
whole selected time range), summed in Float64 and rounded once.  `mask`: `nothing`
or a `UInt8` array of the window's size, any axis of which may be 1; a byte of 0
keeps the sample.  `data` is `Float32` `(nfpc, ni, nto)`, `kept` `Int32`."""
function gpu_fold(A::Array{Float32,3}, nfpc::Integer; tavby=nothing, f=mean, mask=nothing,
                  idxs::Tuple=(:, :, :), dev::Integer=0)
    op = _maskedop(f)
    win = window(idxs, size(A))
    shp, T = _fold_shape(size(A), win, nfpc, tavby)
    ld = mask === nothing ? Int64[] : _mask_ld(mask, (win[2], win[5], win[8]))
    mptr = mask === nothing ? Ptr{UInt8}(C_NULL) : pointer(mask)
    ldp = mask === nothing ? Ptr{Int64}(C_NULL) : pointer(ld)
    data = Array{Float32,3}(undef, shp...)
    kept = Array{UInt32,3}(undef, shp...)
    GC.@preserve A mask win ld data kept check(ccall((:bldp_fold_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{UInt8},
         Ptr{Int64}, Ptr{Float32}, Ptr{UInt32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, nfpc, T, op, mptr, ldp, data, kept))
    data, Int32.(kept)   # counts are < 2^31
end

"""
    gpu_fold(in::Ptr{Float32}, dims, nfpc, tavby, mask::Ptr{UInt8}, out, kept; f=mean,
             win=C_NULL, mask_ld=C_NULL, out_ld=nothing, stream=C_NULL)

The same on DEVICE memory (bldp_fold_f32; asynchronous on `stream`): `mask` may be
`C_NULL` (everything is kept); element (k, i, t') of `out` and `kept` at
`[k + i*out_ld[1] + t'*out_ld[2]]` (dense by default).  `out` or `kept` may be
`C_NULL`, not both.  Returns the dims of the outputs."""
function gpu_fold(in::Ptr{Float32}, dims::NTuple{3,Integer}, nfpc::Integer, tavby::Integer,
                  mask::Ptr{UInt8}, out::Ptr{Float32}, kept::Ptr{UInt32}; f=mean,
                  win=Ptr{Int64}(C_NULL), mask_ld=Ptr{Int64}(C_NULL), out_ld=nothing,
                  stream::Ptr{Cvoid}=C_NULL)
    op = _maskedop(f)
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_fold_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        dims[1], dims[2], dims[3], win, nfpc, tavby, shp))
    ld = out_ld === nothing ? (shp[1], shp[1] * shp[2]) : out_ld
    GC.@preserve win mask_ld check(ccall((:bldp_fold_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{UInt8},
         Ptr{Int64}, Ptr{Float32}, Ptr{UInt32}, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, nfpc, tavby, op, mask, mask_ld, out, kept, ld[1],
        ld[2], stream))
    (shp[1], shp[2], shp[3])
end

"""
    gpu_fold_plan(dims, nfpc, tavby; win=C_NULL, mask_ld=C_NULL) -> NamedTuple

The launch plan of `gpu_fold` on aligned device memory (bldp_fold_plan_f32;
launches nothing and needs no GPU).  `mask_ld = C_NULL`: no mask."""
function gpu_fold_plan(dims::NTuple{3,Integer}, nfpc::Integer, tavby::Integer;
                       win=Ptr{Int64}(C_NULL), mask_ld=Ptr{Int64}(C_NULL))
    info = zeros(Int64, 10)
    GC.@preserve win mask_ld info check(ccall((:bldp_fold_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{UInt8}, Ptr{Int64},
         Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, nfpc, tavby, C_NULL, mask_ld, info))
    (path = (:cols, :rows)[info[1] + 1], channel_lanes = info[2], chunks_per_block = info[3],
     workgroups = info[4], workspace_bytes = info[5], launches = info[6],
     mask_loads = (:byte, :dword, :row, :none)[info[7] + 1], vector_loads = info[8] != 0,
     outputs = info[9], units_per_chunk = info[10])
end

"""
    gpu_band_fold(banks::Vector{Ptr{Float32}}, dims, nfpc, tavby, mask, out, kept; f=mean,
                  win=C_NULL, mask_ld=C_NULL, stream=C_NULL)

The fold of a band resident on one GPU (bldp_band_fold_f32): ONE dense
`(nfpc, ni, nto)` profile over the coarse channels of every bank, not a vcat; bank
b's channel c is channel `b*nc + c` of the mask."""
function gpu_band_fold(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer}, nfpc::Integer,
                       tavby::Integer, mask::Ptr{UInt8}, out::Ptr{Float32}, kept::Ptr{UInt32};
                       f=mean, win=Ptr{Int64}(C_NULL), mask_ld=Ptr{Int64}(C_NULL),
                       stream::Ptr{Cvoid}=C_NULL)
    op = _maskedop(f)
    GC.@preserve banks win mask_ld check(ccall((:bldp_band_fold_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint,
         Ptr{UInt8}, Ptr{Int64}, Ptr{Float32}, Ptr{UInt32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, nfpc, tavby, op, mask, mask_ld,
        out, kept, stream))
    nothing
end

"""
    gpu_unfold(A::Array{Float32,3}, prof::Array{Float32,3}, nfpc; tavby=nothing,
               how=:divide, idxs=(:,:,:), dev=0) -> Array{Float32,3}

`A[idxs...]` with the profile taken out on GPU `dev` (bldp_unfold_host_f32):
element (c, i, t) divided by (`:divide`) or less (`:subtract`)
`prof[c mod nfpc, i, t div tavby]` (1-based: `prof[mod(c-1, nfpc)+1, i, div(t-1, tavby)+1]`),
one rounded Float32 operation.  `prof` is `gpu_fold`'s `data`."""
function gpu_unfold(A::Array{Float32,3}, prof::Array{Float32,3}, nfpc::Integer; tavby=nothing,
                    how::Symbol=:divide, idxs::Tuple=(:, :, :), dev::Integer=0)
    uop = _unfoldop(how)
    win = window(idxs, size(A))
    shp, T = _fold_shape(size(A), win, nfpc, tavby)
    size(prof) == (shp[1], shp[2], shp[3]) ||
        throw(DimensionMismatch("profile $(size(prof)) is not $((shp[1], shp[2], shp[3]))"))
    out = Array{Float32,3}(undef, win[2], win[5], win[8])
    GC.@preserve A prof win out check(ccall((:bldp_unfold_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{Float32},
         Ptr{Float32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, nfpc, T, uop, prof, out))
    out
end

"""
    gpu_unfold(in::Ptr{Float32}, dims, nfpc, tavby, prof::Ptr{Float32}, prof_ld, out, out_ld;
               how=:divide, win=C_NULL, stream=C_NULL)

The same on DEVICE memory (bldp_unfold_f32; asynchronous on `stream`, one launch):
`prof[k + prof_ld[1]*i + prof_ld[2]*t']`, `out[c + out_ld[1]*i + out_ld[2]*t]`
(0-based), so a bank can write its slot of a stitched band.  Not in place."""
function gpu_unfold(in::Ptr{Float32}, dims::NTuple{3,Integer}, nfpc::Integer, tavby::Integer,
                    prof::Ptr{Float32}, prof_ld::NTuple{2,Integer}, out::Ptr{Float32},
                    out_ld::NTuple{2,Integer}; how::Symbol=:divide, win=Ptr{Int64}(C_NULL),
                    stream::Ptr{Cvoid}=C_NULL)
    uop = _unfoldop(how)
    GC.@preserve win check(ccall((:bldp_unfold_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{Float32}, Int64,
         Int64, Ptr{Float32}, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, nfpc, tavby, uop, prof, prof_ld[1], prof_ld[2], out,
        out_ld[1], out_ld[2], stream))
    nothing
end

"""
    gpu_band_unfold(banks::Vector{Ptr{Float32}}, dims, nfpc, tavby, prof, prof_ld, out;
                    how=:divide, win=C_NULL, stream=C_NULL)

The unfold of every bank of a band resident on one GPU in one launch
(bldp_band_unfold_f32) with ONE profile: `out` holds the dense vcat
`(nbank*nc, ni, nt)`."""
function gpu_band_unfold(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer}, nfpc::Integer,
                         tavby::Integer, prof::Ptr{Float32}, prof_ld::NTuple{2,Integer},
                         out::Ptr{Float32}; how::Symbol=:divide, win=Ptr{Int64}(C_NULL),
                         stream::Ptr{Cvoid}=C_NULL)
    uop = _unfoldop(how)
    GC.@preserve banks win check(ccall((:bldp_band_unfold_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint,
         Ptr{Float32}, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, nfpc, tavby, uop, prof, prof_ld[1],
        prof_ld[2], out, stream))
    nothing
end

# ---- dedoppler: bldp_*dedoppler_* (the drift-rate sums of every channel) ----
"""
    gpu_dedoppler(A::Array{Float32,3}, maxdrift; tavby=nothing, seg=0, idxs=(:,:,:), dev=0,
                  sums=false) -> (best, drift[, sums])

The drift-rate sums of every channel of `A[idxs...]` on GPU `dev`
(bldp_dedoppler_host_f32; the rule of include/bldp.h): `tavby` spectra make a block
(`nothing`: the whole selected time range), drift d in `-maxdrift:maxdrift` moves
`sign(d) * fld(2|d|t + T-1, 2(T-1))` selected channels at spectrum t of a block, and
a sum adds the block's samples along that path in Float32, in time order, inside
the segment of `seg` channels that holds the channel (`0`: the whole window).
`best` is `Float32` `(nc, ni, nb)`, the greatest sum of every channel; `drift`
`Int32`, the d it belongs to; with `sums=true` also the `(nc, ni, nb, 2maxdrift+1)`
sums, plane `d + maxdrift + 1`."""
function gpu_dedoppler(A::Array{Float32,3}, maxdrift::Integer; tavby=nothing, seg::Integer=0,
                       idxs::Tuple=(:, :, :), dev::Integer=0, sums::Bool=false)
    win = window(idxs, size(A))
    T = tavby === nothing ? max(win[8], 1) : Int64(tavby)
    T >= 2 || throw(ArgumentError("dedoppler: tavby=$T: a block needs two spectra"))
    win[8] % T == 0 ||
        throw(DimensionMismatch("tavby=$T does not divide ntime=$(win[8])"))
    shp = (win[2], win[5], win[8] ÷ T)
    best = Array{Float32,3}(undef, shp...)
    drift = Array{Cint,3}(undef, shp...)
    S = sums ? Array{Float32,4}(undef, shp..., 2 * maxdrift + 1) : nothing
    sptr = sums ? pointer(S) : Ptr{Float32}(C_NULL)
    GC.@preserve A win best drift S check(ccall((:bldp_dedoppler_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Int64, Ptr{Float32},
         Ptr{Cint}, Ptr{Float32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, T, maxdrift, seg, best, drift, sptr))
    sums ? (best, Int32.(drift), S) : (best, Int32.(drift))
end

"""
    gpu_dedoppler(in::Ptr{Float32}, dims, tavby, maxdrift, best, drift, sums; seg=0,
                  win=C_NULL, out_ld, stream=C_NULL)

The same on DEVICE memory (bldp_dedoppler_f32; asynchronous on `stream`, one
launch): element (c, i, b) of `best` and `drift` at `[c + i*out_ld[1] + b*out_ld[2]]`,
plane k of `sums` at `+ k*out_ld[3]`.  `best` and `drift` go together; that pair or
`sums` may be `C_NULL`, not both."""
function gpu_dedoppler(in::Ptr{Float32}, dims::NTuple{3,Integer}, tavby::Integer,
                       maxdrift::Integer, best::Ptr{Float32}, drift::Ptr{Cint},
                       sums::Ptr{Float32}; seg::Integer=0, win=Ptr{Int64}(C_NULL),
                       out_ld::NTuple{3,Integer}, stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve win check(ccall((:bldp_dedoppler_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Int64, Ptr{Float32},
         Ptr{Cint}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Cvoid}),
        in, dims[1], dims[2], dims[3], win, tavby, maxdrift, seg, best, drift, sums, out_ld[1],
        out_ld[2], out_ld[3], stream))
    nothing
end

"""
    gpu_dedoppler_plan(dims, tavby, maxdrift; seg=0, win=C_NULL) -> NamedTuple

The launch plan of `gpu_dedoppler` on aligned device memory
(bldp_dedoppler_plan_f32; launches nothing and needs no GPU)."""
function gpu_dedoppler_plan(dims::NTuple{3,Integer}, tavby::Integer, maxdrift::Integer;
                            seg::Integer=0, win=Ptr{Int64}(C_NULL))
    info = zeros(Int64, 10)
    GC.@preserve win info check(ccall((:bldp_dedoppler_plan_f32, libbldp), Cint,
        (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Int64, Ptr{Int64}),
        C_NULL, dims[1], dims[2], dims[3], win, tavby, maxdrift, seg, info))
    (path = (:resident, :chunked)[info[1] + 1], tile_channels = info[2], halo = info[3],
     rows_per_chunk = info[4], drifts_per_group = info[5], groups = info[6],
     lds_bytes = info[7], workgroups = info[8], vector_loads = info[9] != 0,
     workspace_bytes = info[10])
end

"""
    gpu_band_dedoppler(banks::Vector{Ptr{Float32}}, dims, tavby, maxdrift, best, drift, sums;
                       seg=0, win=C_NULL, stream=C_NULL)

The dedoppler of every bank of a band resident on one GPU in one launch
(bldp_band_dedoppler_f32): dense outputs, the vcat `(nbank*nc, ni, nb[, K])` of the
banks'.  Segments are counted from each bank's first selected channel."""
function gpu_band_dedoppler(banks::Vector{Ptr{Float32}}, dims::NTuple{3,Integer},
                            tavby::Integer, maxdrift::Integer, best::Ptr{Float32},
                            drift::Ptr{Cint}, sums::Ptr{Float32}; seg::Integer=0,
                            win=Ptr{Int64}(C_NULL), stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve banks win check(ccall((:bldp_band_dedoppler_f32, libbldp), Cint,
        (Cint, Ptr{Ptr{Float32}}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Int64,
         Ptr{Float32}, Ptr{Cint}, Ptr{Float32}, Ptr{Cvoid}),
        length(banks), banks, dims[1], dims[2], dims[3], win, tavby, maxdrift, seg, best, drift,
        sums, stream))
    nothing
end

# fqavfunc values whose result is a position (csrc/argext.hip, enum bldp_argop)
argcode(f) = f === argmax ? Cint(0) : f === argmin ? Cint(1) : nothing

"""
    gpu_argext(A::Array{Float32,3}, fqavby, tavby=1; f=argmax, idxs=(:,:,:), dev=0, values=false)

Where in each `fqavby` x `tavby` block of `A[idxs...]` the extreme lies, computed
on GPU `dev` (bldp_argext_host_f32): an `Array{Int32,3}` of 1-based offsets
`k + fqavby * (tt - 1)` into the block in column-major order, i.e. the linear
index of `argmax(reshape(block, fqavby, tavby))`: the first of the
isless-greatest (`f=argmin`: least) elements, and the first NaN when the block
holds one.  `values=true` returns `(vals, offs)` as `findmax` orders them,
`vals` being the elements at the offsets."""
function gpu_argext(A::Array{Float32,3}, fqavby::Integer, tavby::Integer=1;
                    f=argmax, idxs::Tuple=(:, :, :), dev::Integer=0, values::Bool=false)
    op = argcode(f)
    op === nothing && throw(ArgumentError("gpu_argext takes argmax or argmin, not $f"))
    win = window(idxs, size(A))
    shp = zeros(Int64, 3)
    GC.@preserve win check(ccall((:bldp_reduce_shape, libbldp), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, shp))
    idx = Array{UInt32,3}(undef, shp...)
    val = values ? Array{Float32,3}(undef, shp...) : nothing
    vp = values ? pointer(val) : Ptr{Float32}(C_NULL)
    GC.@preserve A win idx val check(ccall((:bldp_argext_host_f32, libbldp), Cint,
        (Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Int64, Int64, Cint, Ptr{UInt32},
         Ptr{Float32}),
        dev, A, size(A, 1), size(A, 2), size(A, 3), win, fqavby, tavby, op, idx, vp))
    offs = Int32.(idx) .+ Int32(1)   # 0-based offsets < 2^31 -> Julia's 1-based
    values ? (val, offs) : offs
end

"""
    getdata(A::Array; idxs=(:,:,:), fqavby=1, fqavfunc=sum, tavby=1, tavfunc=nothing, dev=0)

WorkerFunctions.getdata's reduction (src/gbtworkerfunctions.jl:191-195) of an
array the worker has read, on GPU `dev`.  `tavfunc === nothing`: `fqavfunc`
reduces the fqavby x tavby block (gpu_fqav).  `tavfunc` given: the time
integration takes its own function,
`tav(fqav(A[idxs...], fqavby; f=fqavfunc), tavby; f=tavfunc)`; either stage is
skipped when its factor is <= 1.  var / std / median / mad of Float32 data run in
gpu_tstat, sum / mean / maximum / minimum in gpu_reduce, anything else (other
element types, other functions) in Julia on the host.  `fqavfunc === argmax` /
`argmin` of Float32 data with `tavby <= 1` run in gpu_argext and return the
`CartesianIndex(k, c', i, t)` array the reference's fqav returns."""
function getdata(A::Array{T,3}; idxs::Tuple=(:, :, :), fqavby::Integer=1, fqavfunc=sum,
                 tavby::Integer=1, tavfunc=nothing, dev::Integer=0) where {T}
    W = all(i -> i isa Colon, idxs) ? A : A[map(i -> i isa Integer ? (i:i) : i, idxs)...]
    if argcode(fqavfunc) !== nothing && W isa Array{Float32,3} && tavby <= 1 && fqavby > 1
        # fqav(W, fqavby; f=argmax) is argmax(reshape(W, fqavby, :, ni, nt); dims=1)
        # with dims=1 dropped: the CartesianIndex (k, c', i, t) of each block's winner
        tavfunc === nothing || throw(ArgumentError("argmax / argmin take no tavfunc"))
        offs = gpu_argext(W, fqavby; f=fqavfunc, dev)
        return [CartesianIndex(Int(offs[I]), I[1], I[2], I[3]) for I in CartesianIndices(offs)]
    end
    tavfunc === nothing && return gpu_fqav(W, fqavby; f=fqavfunc, tavby, dev)
    B = gpu_fqav(W, fqavby; f=fqavfunc, dev)
    tavby <= 1 && return B
    size(B, 3) % tavby == 0 ||
        throw(DimensionMismatch("tavby=$tavby does not divide ntime=$(size(B, 3))"))
    if B isa Array{Float32,3} && statcode(tavfunc) !== nothing
        return gpu_tstat(B, tavby; f=tavfunc, dev)
    elseif B isa Array{<:GPUElt,3} && opcode(tavfunc) !== nothing
        return gpu_reduce(B, 1, tavby; f=tavfunc, dev)
    end
    R = reshape(B, size(B, 1), size(B, 2), tavby, :)
    dropdims(tavfunc(R, dims=3), dims=3)
end

"""
    getband(parts; idxs=(:,:,:), fqavby=1, fqavfunc=sum, tavby=1, tavfunc=nothing, dev=0)

`reduce(vcat, ...)` of `getdata` of every bank's array, in bank order
(src/gbt.jl:103)."""
function getband(parts::AbstractVector; idxs::Tuple=(:, :, :), fqavby::Integer=1, fqavfunc=sum,
                 tavby::Integer=1, tavfunc=nothing, dev::Integer=0)
    reduce(vcat, [getdata(A; idxs, fqavby, fqavfunc, tavby, tavfunc, dev) for A in parts])
end

"""
    gpu_band(parts) -> Array{Float32,3}

`reduce(vcat, parts)` of per-bank results in bank order (src/gbt.jl:103):
what `GBT.getband` returns after `fetch.(futures)`."""
gpu_band(parts) = reduce(vcat, parts)

# ---------------------------------------------------------------------------
# Band stitch across worker processes, one GPU each, over RCCL (xGMI): the
# device-side replacement of GBT.getdata's fetch of every worker's result
# (src/gbt.jl:75-78).  The 128-byte id travels between workers through
# Distributed (e.g. `remotecall_fetch(gpu_comm_id, first(workers))`).

"RCCL unique id for a new band communicator (call on one worker)."
function gpu_comm_id()
    id = zeros(UInt8, 128)
    check(ccall((:bldp_comm_id, libbldp), Cint, (Ptr{UInt8},), id))
    id
end

"Join the band communicator (collective over all `nranks` workers)."
function gpu_comm_init(id::Vector{UInt8}, nranks::Integer, rank::Integer; dev::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:bldp_comm_init, libbldp), Cint, (Cint, Cint, Cint, Ptr{UInt8}, Ptr{Ptr{Cvoid}}),
                dev, nranks, rank, id, h))
    h[]
end

gpu_comm_destroy(comm::Ptr{Cvoid}) =
    (check(ccall((:bldp_comm_destroy, libbldp), Cint, (Ptr{Cvoid},), comm)); nothing)

"""
    gpu_band_gather(comm, slice::Ptr{Float32}, count, gathered::Ptr{Float32}; root=0, stream=C_NULL)

ncclGather of every worker's reduced slice (a device buffer of `count`
Float32, its banks in vcat order) into `gathered` (nranks*count) on `root`,
rank-major; then `bldp_stitch_f32` when the product has more than one
(IF, time) row.  Device pointers; asynchronous on `stream`."""
gpu_band_gather(comm::Ptr{Cvoid}, slice::Ptr{Float32}, count::Integer, gathered::Ptr{Float32};
                root::Integer=0, stream::Ptr{Cvoid}=C_NULL) =
    (check(ccall((:bldp_band_gather_f32, libbldp), Cint,
                 (Ptr{Cvoid}, Cint, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Cvoid}),
                 comm, root, slice, count, gathered, stream)); nothing)

end # module
