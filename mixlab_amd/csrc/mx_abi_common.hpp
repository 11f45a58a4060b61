// mx_abi_common.hpp -- what every mx_abi*.cpp shares (internal): the graph handle and the fence of the extern "C" boundary.
//
// Convention (mirrors the reference's own FFI fencing, codec/src/ffmpeg/ioctx.rs:51-67,136-152):
// nothing unwinds across the boundary; every entry point catches, stashes the message in a
// thread-local, and returns a negative status.
#pragma once
#include <memory>
#include <new>
#include <string>

#include "mx_engine.hpp"

struct mx_graph { std::unique_ptr<mx::Graph> g; };

namespace mx { hipStream_t abi_video_stream(void* stream); }   // mx_abi_video.cpp: a pixel call's stream (NULL: the library's default video stream), its deferred scaler work flushed
void mx_set_last_error(const std::string& s);   // mx_abi.cpp: the one writer of the thread-local behind mx_last_error

template <class F>
static int guard(F&& f) noexcept {
    try {
        f();
        return MX_OK;
    } catch (const mx::Error& e) {
        mx_set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        mx_set_last_error("host allocation failed");
        return MX_ERR_NOMEM;
    } catch (const std::exception& e) {
        mx_set_last_error(std::string("internal error: ") + e.what());
        return MX_ERR_INTERNAL;
    } catch (...) {
        mx_set_last_error("internal error: unknown exception");
        return MX_ERR_INTERNAL;
    }
}

#define REQUIRE(cond, msg) do { if (!(cond)) throw mx::Error(MX_ERR_INVALID, msg); } while (0)
