/* GL/glew.h stand-in for tools/scale_gl_run.c: GLEW is not needed to run the `scale` postprocessor on Mesa llvmpipe.  The GL entry points
 * the module calls are routed through pointers that scale_gl_run.c fills from the context it made current (_glapi_get_proc_address),
 * so the module's text compiles unmodified and no libGL is linked. */
#ifndef SCALE_GL_SHIM_GLEW_H
#define SCALE_GL_SHIM_GLEW_H

#define GL_GLEXT_PROTOTYPES 1
#include <GL/gl.h>
#include <GL/glext.h>

#define SCALE_GL_FUNCS(X)                                                                                                                     \
        X(glEnable) X(glGenTextures) X(glBindTexture) X(glTexParameteri) X(glTexImage2D) X(glTexSubImage2D) X(glGenFramebuffers)            \
        X(glBindFramebuffer) X(glFramebufferTexture2D) X(glViewport) X(glClearColor) X(glClear) X(glBegin) X(glTexCoord2f) X(glVertex2f) \
        X(glEnd) X(glReadPixels) X(glDeleteTextures) X(glDeleteFramebuffers) X(glGetError) X(glFinish) X(glGetString)

#define SCALE_GL_DECLARE(name) extern __typeof__(&name) p_##name;
SCALE_GL_FUNCS(SCALE_GL_DECLARE)
#undef SCALE_GL_DECLARE

#define glEnable p_glEnable
#define glGenTextures p_glGenTextures
#define glBindTexture p_glBindTexture
#define glTexParameteri p_glTexParameteri
#define glTexImage2D p_glTexImage2D
#define glTexSubImage2D p_glTexSubImage2D
#define glGenFramebuffers p_glGenFramebuffers
#define glBindFramebuffer p_glBindFramebuffer
#define glFramebufferTexture2D p_glFramebufferTexture2D
#define glViewport p_glViewport
#define glClearColor p_glClearColor
#define glClear p_glClear
#define glBegin p_glBegin
#define glTexCoord2f p_glTexCoord2f
#define glVertex2f p_glVertex2f
#define glEnd p_glEnd
#define glReadPixels p_glReadPixels
#define glDeleteTextures p_glDeleteTextures
#define glDeleteFramebuffers p_glDeleteFramebuffers
#define glGetError p_glGetError
#define glFinish p_glFinish
#define glGetString p_glGetString

#endif
